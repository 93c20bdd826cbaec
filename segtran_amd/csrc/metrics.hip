// metrics.hip -- surface-distance metrics of the 3-D evaluation: what medpy.metric.binary.asd / hd95 compute for
// calculate_metric_percase (test_util3d.py:203-206), with unit voxel spacing and connectivity 1, as three image-sized integer kernels:
//   surface_border   border(m) = m XOR erode(m), face neighbourhood, out-of-array neighbours unset (medpy __surface_distances: binary_erosion, border_value 0)
//   edt_sq           the exact squared Euclidean distance to the nearest border voxel (scipy distance_transform_edt of the complement, squared), separable:
//                    one pass per axis, out[y] = min over y' of (f[y'] + (y - y')^2) over the WHOLE line -- O(extent) per voxel, no envelope bookkeeping, int32
//   surface_hist     hist[plane][k] = number of border voxels of the other mask at squared distance k (integer atomic adds: order-independent, bit-reproducible)
// The float64 finish (mean of sqrt(k) weighted by the counts, the 95th percentile from the cumulative counts) is a few lines on the host (infer3d.py).
// And the tail of one BraTS case (test_util3d.py:36-38, 67, 82-85) in one pass over the voxels:
//   brats_case_tail  counts[c-1] = {sum pred * gt, sum pred, sum gt} for the three foreground classes, the ground truth mapped from the raw labels in registers, and
//                    labels = argmax(brats_inv_map_label(soft)) with 3 written as 4.  int32 counts through integer atomic adds: exact, order-independent.
// The one-hot tasks' tail (onehot_case_tail) and the n-hot 2-D tasks' (nhot_case_tail: fundus, polyp) follow the same scheme, one grid row per image.
#include "resample.h"
#include "harden.h"

namespace segx {

constexpr int EDT_INF = SEGX_EDT_INF, EDT_MAX = SEGX_EDT_MAX_EXTENT;
constexpr int EDT_SLAB = 32;                 // consecutive cells of the contiguous axis a workgroup of an H / D pass owns: 128-byte global rows, one bank each in LDS
constexpr int HIST_LOW = 1024;               // bins a workgroup of surface_hist keeps in LDS (distances below 32 voxels: where surfaces that nearly agree pile up)

// border[p][z][y][x] = set && !(every face neighbour set); a neighbour outside the array is unset.  nd == 2: the z neighbours do not exist (a stack of images).
// One thread per voxel.
__global__ __launch_bounds__(256) void surface_border_kernel(const float* __restrict__ mask, uint8_t* __restrict__ border, int64_t planes, int D, int H, int W,
                                                             int nd) {
    const int64_t HW = (int64_t)H * W, total = planes * D * HW;
    for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * 256) {
        int64_t r = idx % ((int64_t)D * HW);
        const int z = (int)(r / HW); r -= (int64_t)z * HW;
        const int y = (int)(r / W), x = (int)(r - (int64_t)y * W);
        bool b = false;
        if (mask[idx] != 0.0f) {
            bool in = x > 0 && x < W - 1 && y > 0 && y < H - 1 && (nd == 2 || (z > 0 && z < D - 1));
            if (in) {
                in = mask[idx - 1] != 0.0f && mask[idx + 1] != 0.0f && mask[idx - W] != 0.0f && mask[idx + W] != 0.0f;
                if (in && nd == 3) in = mask[idx - HW] != 0.0f && mask[idx + HW] != 0.0f;
            }
            b = !in;
        }
        border[idx] = b ? 1 : 0;
    }
}

// W pass: d2[row][x] = min over x' with border[row][x'] set of (x - x')^2, EDT_INF for a row without one.  A wave owns a row (staged in LDS as 0 / EDT_INF; every
// lane reads the same x': a broadcast) and a lane up to four cells of it, 64 apart: W <= 256.
__global__ __launch_bounds__(256) void edt_row_kernel(const uint8_t* __restrict__ border, int* __restrict__ d2, int64_t rows, int W) {
    __shared__ int f[4 * EDT_MAX];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    int* fr = f + wave * EDT_MAX;
    for (int64_t row0 = (int64_t)blockIdx.x * 4; row0 < rows; row0 += (int64_t)gridDim.x * 4) {
        const int64_t row = row0 + wave;
        if (row < rows)
            for (int x = lane; x < W; x += 64) fr[x] = border[row * W + x] ? 0 : EDT_INF;
        __syncthreads();
        if (row < rows) {
            int o0 = EDT_INF, o1 = EDT_INF, o2 = EDT_INF, o3 = EDT_INF;
            for (int xp = 0; xp < W; ++xp) {
                const int v = fr[xp], t = lane - xp;
                o0 = min(o0, v + t * t); o1 = min(o1, v + (t + 64) * (t + 64)); o2 = min(o2, v + (t + 128) * (t + 128)); o3 = min(o3, v + (t + 192) * (t + 192));
            }
            int* o = d2 + row * W;
            if (lane < W) o[lane] = min(o0, EDT_INF);
            if (lane + 64 < W) o[lane + 64] = min(o1, EDT_INF);
            if (lane + 128 < W) o[lane + 128] = min(o2, EDT_INF);
            if (lane + 192 < W) o[lane + 192] = min(o3, EDT_INF);
        }
        __syncthreads();
    }
}

// H / D pass, in place, on g viewed as [outer][n][inner] (inner contiguous): g[o][y][x] = min(EDT_INF, min over y' of (g[o][y'][x] + (y - y')^2)).  A workgroup owns
// the n lines of EDT_SLAB consecutive x of one o, staged in LDS as [n][EDT_SLAB]: global rows of 128 bytes, LDS reads across lanes in x (32 banks, the two halves of a
// wave read the same addresses).  A thread computes four consecutive outputs of its column per sweep over the line, so one LDS read feeds four add / min pairs.
// It reads the LDS copy and writes only global memory: in place is safe, the slab is this workgroup's alone.
__global__ __launch_bounds__(256) void edt_axis_kernel(int* __restrict__ g, int64_t outer, int n, int64_t inner) {
    __shared__ int f[EDT_MAX * EDT_SLAB];
    const int64_t slabs = (inner + EDT_SLAB - 1) / EDT_SLAB, items = outer * slabs;
    const int tx = threadIdx.x & (EDT_SLAB - 1), ty = threadIdx.x / EDT_SLAB;
    for (int64_t item = blockIdx.x; item < items; item += gridDim.x) {
        const int64_t o = item / slabs, x = (item - o * slabs) * EDT_SLAB + tx;
        int* col = g + o * n * inner + x;
        for (int y = ty; y < n; y += 256 / EDT_SLAB) f[y * EDT_SLAB + tx] = x < inner ? col[(int64_t)y * inner] : EDT_INF;
        __syncthreads();
        for (int y0 = ty * 4; y0 < n; y0 += 4 * (256 / EDT_SLAB)) {
            int o0 = EDT_INF, o1 = EDT_INF, o2 = EDT_INF, o3 = EDT_INF;
            for (int yp = 0; yp < n; ++yp) {
                const int v = f[yp * EDT_SLAB + tx], t = y0 - yp;
                o0 = min(o0, v + t * t); o1 = min(o1, v + (t + 1) * (t + 1)); o2 = min(o2, v + (t + 2) * (t + 2)); o3 = min(o3, v + (t + 3) * (t + 3));
            }
            if (x < inner) {
                col[(int64_t)y0 * inner] = min(o0, EDT_INF);
                if (y0 + 1 < n) col[(int64_t)(y0 + 1) * inner] = min(o1, EDT_INF);
                if (y0 + 2 < n) col[(int64_t)(y0 + 2) * inner] = min(o2, EDT_INF);
                if (y0 + 3 < n) col[(int64_t)(y0 + 3) * inner] = min(o3, EDT_INF);
            }
        }
        __syncthreads();
    }
}

// hist[plane][k] += 1 for every voxel of border[plane] whose d2[plane] is k < nbins.  blockIdx.y = plane; the low bins are counted in LDS and added to global
// memory once per workgroup, the rest go to global memory directly.
__global__ __launch_bounds__(256) void surface_hist_kernel(const uint8_t* __restrict__ border, const int* __restrict__ d2, int* __restrict__ hist, int64_t S,
                                                           int nbins) {
    __shared__ int low[HIST_LOW];
    const int plane = blockIdx.y;
    const uint8_t* b = border + (int64_t)plane * S; const int* d = d2 + (int64_t)plane * S; int* h = hist + (int64_t)plane * nbins;
    for (int i = threadIdx.x; i < HIST_LOW; i += 256) low[i] = 0;
    __syncthreads();
    for (int64_t s = (int64_t)blockIdx.x * 256 + threadIdx.x; s < S; s += (int64_t)gridDim.x * 256) {
        if (!b[s]) continue;
        const unsigned k = (unsigned)d[s];
        if (k >= (unsigned)nbins) continue;
        if (k < (unsigned)HIST_LOW) atomicAdd(&low[k], 1);
        else atomicAdd(&h[k], 1);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < HIST_LOW && i < nbins; i += 256)
        if (low[i]) atomicAdd(&h[i], low[i]);
}

constexpr int CT_THREADS = SEGX_CASE_TAIL_THREADS, CT_WAVES = CT_THREADS / 64;

__global__ __launch_bounds__(64) void case_tail_init_kernel(int* __restrict__ counts) {
    if (threadIdx.x < 9) counts[threadIdx.x] = 0;
}

__device__ __forceinline__ int wave_sum_int(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// argmax over k of inv[k] as torch.argmax takes it: the lowest index wins a tie, a NaN beats every number (and the first NaN the later ones)
__device__ __forceinline__ bool case_tail_beats(float v, float best) { return v > best || (v != v && best == best); }

// soft / hard [4][S] (bg, ET, WT, TC; plane 0 is never read), gt [S] raw labels.  A thread owns four consecutive voxels per trip of the grid-stride loop.  VEC: S % 4 == 0
// and every operand aligned for it, so a plane's quad is one 16-byte load and the four labels one 4-byte store; otherwise dword loads and byte stores, the last quad
// cut at S.  counts == NULL: hard and gt are not read; labels == NULL: soft is not read (both conditions are the same in every thread of the grid).
template <bool VEC>
__global__ __launch_bounds__(CT_THREADS) void brats_case_tail_kernel(const float* __restrict__ soft, const float* __restrict__ hard, const int* __restrict__ gt,
                                                                     int* __restrict__ counts, uint8_t* __restrict__ labels, int64_t S) {
    __shared__ int red[CT_WAVES][9];
    int i1 = 0, p1 = 0, g1 = 0, i2 = 0, p2 = 0, g2 = 0, i3 = 0, p3 = 0, g3 = 0;
    const int64_t quads = (S + 3) >> 2;
    for (int64_t q = (int64_t)blockIdx.x * CT_THREADS + threadIdx.x; q < quads; q += (int64_t)gridDim.x * CT_THREADS) {
        const int64_t s = q << 2;
        const int n = VEC ? 4 : (int)i64min(4, S - s);
        if (counts) {
            float h1[4] = {0.f, 0.f, 0.f, 0.f}, h2[4] = {0.f, 0.f, 0.f, 0.f}, h3[4] = {0.f, 0.f, 0.f, 0.f};
            int g[4] = {0, 0, 0, 0};
            if (VEC) {
                const float4 a = *reinterpret_cast<const float4*>(hard + S + s), b = *reinterpret_cast<const float4*>(hard + 2 * S + s),
                             c = *reinterpret_cast<const float4*>(hard + 3 * S + s);
                const int4 l = *reinterpret_cast<const int4*>(gt + s);
                h1[0] = a.x; h1[1] = a.y; h1[2] = a.z; h1[3] = a.w; h2[0] = b.x; h2[1] = b.y; h2[2] = b.z; h2[3] = b.w;
                h3[0] = c.x; h3[1] = c.y; h3[2] = c.z; h3[3] = c.w; g[0] = l.x; g[1] = l.y; g[2] = l.z; g[3] = l.w;
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (j < n) { h1[j] = hard[S + s + j]; h2[j] = hard[2 * S + s + j]; h3[j] = hard[3 * S + s + j]; g[j] = gt[s + j]; }
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int v = g[j] == 4 ? 3 : g[j];                             // a raw 4 is class 3 (test_util3d.py:36)
                const int et = v == 3, wt = v >= 1 && v <= 3, tc = v == 1 || v == 3;
                const int a = h1[j] != 0.0f, b = h2[j] != 0.0f, c = h3[j] != 0.0f;
                i1 += a & et; p1 += a; g1 += et; i2 += b & wt; p2 += b; g2 += wt; i3 += c & tc; p3 += c; g3 += tc;
            }
        }
        if (labels) {
            float s1[4] = {0.f, 0.f, 0.f, 0.f}, s2[4] = {0.f, 0.f, 0.f, 0.f}, s3[4] = {0.f, 0.f, 0.f, 0.f};
            if (VEC) {
                const float4 a = *reinterpret_cast<const float4*>(soft + S + s), b = *reinterpret_cast<const float4*>(soft + 2 * S + s),
                             c = *reinterpret_cast<const float4*>(soft + 3 * S + s);
                s1[0] = a.x; s1[1] = a.y; s1[2] = a.z; s1[3] = a.w; s2[0] = b.x; s2[1] = b.y; s2[2] = b.z; s2[3] = b.w;
                s3[0] = c.x; s3[1] = c.y; s3[2] = c.z; s3[3] = c.w;
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (j < n) { s1[j] = soft[S + s + j]; s2[j] = soft[2 * S + s + j]; s3[j] = soft[3 * S + s + j]; }
            }
            unsigned lab[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {                                       // brats_inv_map_label (datasets3d.py:65-90): one subtraction, at most one product each
                const float inv0 = 1.0f - s2[j], inv1 = (s3[j] - s1[j]) * 1.5f, inv2 = (s2[j] - s3[j]) * 1.5f, inv3 = s1[j];
                float best = inv0; unsigned k = 0;
                if (case_tail_beats(inv1, best)) { best = inv1; k = 1; }
                if (case_tail_beats(inv2, best)) { best = inv2; k = 2; }
                if (case_tail_beats(inv3, best)) { best = inv3; k = 4; }        // label 3 is exported as 4 (test_util3d.py:84-85)
                lab[j] = k;
            }
            if (VEC) {
                *reinterpret_cast<uint32_t*>(labels + s) = lab[0] | (lab[1] << 8) | (lab[2] << 16) | (lab[3] << 24);
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (j < n) labels[s + j] = (uint8_t)lab[j];
            }
        }
    }
    if (counts) {                                                               // wave -> LDS -> one atomic add per counter per workgroup
        const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
        i1 = wave_sum_int(i1); p1 = wave_sum_int(p1); g1 = wave_sum_int(g1); i2 = wave_sum_int(i2); p2 = wave_sum_int(p2); g2 = wave_sum_int(g2);
        i3 = wave_sum_int(i3); p3 = wave_sum_int(p3); g3 = wave_sum_int(g3);
        if (lane == 0) {
            int* r = red[wave];
            r[0] = i1; r[1] = p1; r[2] = g1; r[3] = i2; r[4] = p2; r[5] = g2; r[6] = i3; r[7] = p3; r[8] = g3;
        }
        __syncthreads();
        if (threadIdx.x < 9) {
            int t = 0;
#pragma unroll
            for (int w = 0; w < CT_WAVES; ++w) t += red[w][threadIdx.x];
            if (t) atomicAdd(counts + threadIdx.x, t);
        }
    }
}

// ---- one-hot tasks (OCT: 10 retinal-layer classes; datasets2d.py:22-86, test_util2d.py:241-265) ----
// out[b][c][s] = (labels[b][s] == c); labels are bytes (BYTES == 1) or int32 (BYTES == 4).  A label outside 0..C-1 matches no class.  One thread per pixel.
template <int BYTES>
__global__ __launch_bounds__(256) void index_onehot_kernel(const void* __restrict__ labels, float* __restrict__ out, int64_t B, int C, int64_t S) {
    const int64_t total = B * S;
    for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * 256) {
        const int64_t b = idx / S, s = idx - b * S;
        const int l = BYTES == 1 ? (int)reinterpret_cast<const uint8_t*>(labels)[idx] : reinterpret_cast<const int*>(labels)[idx];
        float* o = out + b * C * S + s;
        for (int c = 0; c < C; ++c) o[c * S] = l == c ? 1.0f : 0.0f;
    }
}

// out[b][s][0..2] = colormap[argmax_c nhot[b][c][s]] (colormap == NULL: the index itself, three times); the arg-max as torch.argmax takes it (case_tail_beats)
__global__ __launch_bounds__(256) void onehot_colormap_kernel(const float* __restrict__ nhot, const uint8_t* __restrict__ colormap, uint8_t* __restrict__ out,
                                                              int64_t B, int C, int64_t S) {
    const int64_t total = B * S;
    for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * 256) {
        const int64_t b = idx / S, s = idx - b * S;
        const float* src = nhot + b * C * S + s;
        float best = src[0]; int k = 0;
        for (int c = 1; c < C; ++c) {
            const float v = src[c * S];
            if (case_tail_beats(v, best)) { best = v; k = c; }
        }
        uint8_t* o = out + idx * 3;
        if (colormap) { o[0] = colormap[3 * k]; o[1] = colormap[3 * k + 1]; o[2] = colormap[3 * k + 2]; }
        else { o[0] = o[1] = o[2] = (uint8_t)k; }
    }
}

__global__ __launch_bounds__(256) void onehot_tail_init_kernel(int* __restrict__ counts, int n) {
    for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) counts[i] = 0;
}

// The evaluation tail of a one-hot task: soft [B][C][S], gt [B][S] index labels (bytes).  blockIdx.y = image; within it the scheme of brats_case_tail_kernel: a thread
// owns four consecutive pixels per trip of the grid-stride loop, VEC as there (S % 4 == 0 and every operand aligned: a class's quad is one 16-byte load, the four
// ground-truth bytes one dword, the four labels one dword store, the four colours three).  Per class c = 1..C-1: pred = soft[c] >= T (a NaN is off), gt = (label == c);
// the pixel's label is the lowest class that is on, 0 when none is.  MAXC as in infer.hip: constant trip counts under `c < C`, so the 3 (MAXC - 1) counters of a
// thread stay in registers.  counts == NULL: gt is not read; labels == NULL and rgb == NULL: nothing is stored (all three conditions are uniform over the grid).
template <int MAXC, bool VEC>
__global__ __launch_bounds__(CT_THREADS) void onehot_case_tail_kernel(const float* __restrict__ soft, const uint8_t* __restrict__ gt,
                                                                      const uint8_t* __restrict__ colormap, int* __restrict__ counts, uint8_t* __restrict__ labels,
                                                                      uint8_t* __restrict__ rgb, int C, int64_t S, float T) {
    __shared__ int red[CT_WAVES][3 * (MAXC - 1)];
    __shared__ uint32_t cmap[MAXC];                                             // r | g << 8 | b << 16 per class
    const int64_t b = blockIdx.y;
    soft += b * C * S;
    if (rgb) {
        if (threadIdx.x < C) cmap[threadIdx.x] = colormap[3 * threadIdx.x] | ((uint32_t)colormap[3 * threadIdx.x + 1] << 8) | ((uint32_t)colormap[3 * threadIdx.x + 2] << 16);
        __syncthreads();
    }
    int ci[MAXC - 1], cp[MAXC - 1], cg[MAXC - 1];
#pragma unroll
    for (int c = 0; c < MAXC - 1; ++c) { ci[c] = 0; cp[c] = 0; cg[c] = 0; }
    const int64_t quads = (S + 3) >> 2;
    for (int64_t q = (int64_t)blockIdx.x * CT_THREADS + threadIdx.x; q < quads; q += (int64_t)gridDim.x * CT_THREADS) {
        const int64_t s = q << 2;
        const int n = VEC ? 4 : (int)i64min(4, S - s);
        int g[4] = {0, 0, 0, 0};                                                // class 0 is not counted: a cut quad's missing pixels count nowhere
        if (counts) {
            if (VEC) {
                const uint32_t l = *reinterpret_cast<const uint32_t*>(gt + b * S + s);
                g[0] = l & 255; g[1] = (l >> 8) & 255; g[2] = (l >> 16) & 255; g[3] = l >> 24;
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (j < n) g[j] = gt[b * S + s + j];
            }
        }
        unsigned lab[4] = {0, 0, 0, 0};
#pragma unroll
        for (int c = 1; c < MAXC; ++c) {
            if (c < C) {
                float v[4] = {0.f, 0.f, 0.f, 0.f};
                if (VEC) {
                    const float4 a = *reinterpret_cast<const float4*>(soft + c * S + s);
                    v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w;
                } else {
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        if (j < n) v[j] = soft[c * S + s + j];
                }
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int on = (j < n) & (v[j] >= T), hit = g[j] == c;
                    ci[c - 1] += on & hit; cp[c - 1] += on; cg[c - 1] += hit;
                    if (on && lab[j] == 0) lab[j] = c;
                }
            }
        }
        if (labels) {
            if (VEC) {
                *reinterpret_cast<uint32_t*>(labels + b * S + s) = lab[0] | (lab[1] << 8) | (lab[2] << 16) | (lab[3] << 24);
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (j < n) labels[b * S + s + j] = (uint8_t)lab[j];
            }
        }
        if (rgb) {
            const uint32_t k0 = cmap[lab[0]], k1 = cmap[lab[1]], k2 = cmap[lab[2]], k3 = cmap[lab[3]];
            uint8_t* o = rgb + (b * S + s) * 3;
            if (VEC) {                                                          // 12 bytes: r0 g0 b0 r1 | g1 b1 r2 g2 | b2 r3 g3 b3
                uint32_t* o4 = reinterpret_cast<uint32_t*>(o);
                o4[0] = k0 | (k1 << 24); o4[1] = (k1 >> 8) | (k2 << 16); o4[2] = (k2 >> 16) | (k3 << 8);
            } else {
                const uint32_t k[4] = {k0, k1, k2, k3};
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (j < n) { o[3 * j] = (uint8_t)k[j]; o[3 * j + 1] = (uint8_t)(k[j] >> 8); o[3 * j + 2] = (uint8_t)(k[j] >> 16); }
            }
        }
    }
    if (counts) {                                                               // wave -> LDS -> one atomic add per counter per workgroup
        const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
        for (int c = 0; c < MAXC - 1; ++c) {
            if (c < C - 1) {
                const int a = wave_sum_int(ci[c]), p = wave_sum_int(cp[c]), h = wave_sum_int(cg[c]);
                if (lane == 0) { red[wave][3 * c] = a; red[wave][3 * c + 1] = p; red[wave][3 * c + 2] = h; }
            }
        }
        __syncthreads();
        if ((int)threadIdx.x < 3 * (C - 1)) {
            int t = 0;
#pragma unroll
            for (int w = 0; w < CT_WAVES; ++w) t += red[w][threadIdx.x];
            if (t) atomicAdd(counts + b * 3 * (C - 1) + threadIdx.x, t);
        }
    }
}

// ---- n-hot 2-D tasks (fundus: bg / disc / cup, polyp: bg / polyp; test_util2d.py:241-265, datasets2d.py:90-171, utils/losses.py:76-127) ----
struct NhotTail { int C, Cm, gt_map, same; float T; };   // Cm: channels of the raw mask (gt_map 1..3); same: (h, w) == (H, W), soft is read as it is

// counts[0 .. ncounts) = 0 and every (lowest, highest) pair of ext = (H, -1), segx_row_extent's empty extent; either may be NULL
__global__ __launch_bounds__(256) void nhot_tail_init_kernel(int* __restrict__ counts, int ncounts, int* __restrict__ ext, int npairs, int H) {
    const int n = ncounts > npairs ? ncounts : npairs;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
        if (counts && i < ncounts) counts[i] = 0;
        if (ext && i < npairs) { ext[2 * i] = H; ext[2 * i + 1] = -1; }
    }
}

__device__ __forceinline__ int wave_min_int(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = min(v, __shfl_xor(v, o));
    return v;
}
__device__ __forceinline__ int wave_max_int(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = max(v, __shfl_xor(v, o));
    return v;
}

// harden_cell in mode 0 on one pixel's C values, its 0 / 1 planes as bits: bit c = class c is on (bit 0: no other class is)
template <int MAXC>
__device__ __forceinline__ unsigned harden_bits(float* p, int C, float T) {
    float hd[MAXC];
    harden_cell<MAXC>(p, C, 0, T, nullptr, hd, 1);
    unsigned bits = 0;
#pragma unroll
    for (int c = 0; c < MAXC; ++c)
        if (c < C && hd[c] == 1.0f) bits |= 1u << c;
    return bits;
}

// The evaluation tail of an n-hot 2-D task: one pass over the DESTINATION grid [H][W] of image blockIdx.y, the scheme of onehot_case_tail_kernel (a thread owns four
// consecutive pixels per trip of the grid-stride loop; VEC: H * W % 4 == 0 and every operand aligned, so a plane's quad is one 16-byte access and four bytes one dword).
// Per pixel: the C prediction values -- soft itself (t.same) or interp_at of the [h][w] plane, the expression of interp_fwd_kernel, hence SF.interp_linear's bits --
// hardened by harden_cell (mode 0) into bits; the ground truth's bits from the n-hot floats (gt_map 0: >= 0.5) or from the raw fundus / polyp mask bytes (1..3),
// mapped in registers.  From the two bit sets: counts (as onehot_case_tail_kernel), the row extents of classes 1 and 2 of both (per thread min / max of the rows it
// saw, wave shuffles, LDS, one atomicMin / atomicMax per extent per workgroup), the label bytes (values[c] of the last class on) and the hardened floats.
// counts / ext / labels / hard == NULL: not formed; gt == NULL: not read (all uniform over the grid).
template <int MAXC, bool VEC>
__global__ __launch_bounds__(CT_THREADS) void nhot_case_tail_kernel(const float* __restrict__ soft, const void* __restrict__ gt, const int* __restrict__ values,
                                                                    int* __restrict__ counts, int* __restrict__ ext, uint8_t* __restrict__ labels,
                                                                    float* __restrict__ hard, InterpDims q, NhotTail t) {
    __shared__ int red[CT_WAVES][3 * (MAXC - 1)];
    __shared__ int redx[CT_WAVES][8];
    const int C = t.C, W = q.W;
    const int64_t b = blockIdx.y, S = (int64_t)q.H * q.W, ssz = (int64_t)q.h * q.w;
    soft += b * C * ssz;
    const float* gtf = gt && t.gt_map == 0 ? reinterpret_cast<const float*>(gt) + b * C * S : nullptr;
    const uint8_t* gtb = gt && t.gt_map != 0 ? reinterpret_cast<const uint8_t*>(gt) + b * t.Cm * S : nullptr;
    int vals[MAXC];
#pragma unroll
    for (int c = 0; c < MAXC; ++c) vals[c] = (labels && c < C) ? values[c] : 0;
    int ci[MAXC - 1], cp[MAXC - 1], cg[MAXC - 1];
#pragma unroll
    for (int c = 0; c < MAXC - 1; ++c) { ci[c] = 0; cp[c] = 0; cg[c] = 0; }
    int lo[4], hi[4];                                                           // {prediction, ground truth} x {class 1, class 2}
#pragma unroll
    for (int k = 0; k < 4; ++k) { lo[k] = q.H; hi[k] = -1; }
    const int64_t quads = (S + 3) >> 2;
    for (int64_t qd = (int64_t)blockIdx.x * CT_THREADS + threadIdx.x; qd < quads; qd += (int64_t)gridDim.x * CT_THREADS) {
        const int64_t s = qd << 2;
        const int n = VEC ? 4 : (int)i64min(4, S - s);
        int yj[4], xj[4];                                                       // the four pixels' rows and columns
        yj[0] = (int)(s / W); xj[0] = (int)(s - (int64_t)yj[0] * W);
#pragma unroll
        for (int j = 1; j < 4; ++j) {
            const bool wrap = xj[j - 1] + 1 == W;
            xj[j] = wrap ? 0 : xj[j - 1] + 1; yj[j] = yj[j - 1] + (wrap ? 1 : 0);
        }
        unsigned pb[4] = {0, 0, 0, 0}, gb[4] = {0, 0, 0, 0};                    // a cut quad's missing pixels have no bit: they count nowhere
        if (t.same) {
            float v[MAXC][4];
#pragma unroll
            for (int c = 0; c < MAXC; ++c) {
                v[c][0] = v[c][1] = v[c][2] = v[c][3] = 0.0f;
                if (c < C) {
                    if (VEC) {
                        const float4 a = *reinterpret_cast<const float4*>(soft + c * S + s);
                        v[c][0] = a.x; v[c][1] = a.y; v[c][2] = a.z; v[c][3] = a.w;
                    } else {
#pragma unroll
                        for (int j = 0; j < 4; ++j)
                            if (j < n) v[c][j] = soft[c * S + s + j];
                    }
                }
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (j < n) {
                    float p[MAXC];
#pragma unroll
                    for (int c = 0; c < MAXC; ++c) p[c] = v[c][j];
                    pb[j] = harden_bits<MAXC>(p, C, t.T);
                }
            }
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (j < n) {
                    float p[MAXC];
#pragma unroll
                    for (int c = 0; c < MAXC; ++c) {
                        p[c] = 0.0f;
                        if (c < C) p[c] = interp_at(soft + c * ssz, q, 0, yj[j], xj[j]);
                    }
                    pb[j] = harden_bits<MAXC>(p, C, t.T);
                }
            }
        }
        if (gtf) {                                                              // n-hot floats: class c is on where the value is >= 0.5
#pragma unroll
            for (int c = 1; c < MAXC; ++c) {
                if (c < C) {
                    float g[4] = {0.f, 0.f, 0.f, 0.f};
                    if (VEC) {
                        const float4 a = *reinterpret_cast<const float4*>(gtf + c * S + s);
                        g[0] = a.x; g[1] = a.y; g[2] = a.z; g[3] = a.w;
                    } else {
#pragma unroll
                        for (int j = 0; j < 4; ++j)
                            if (j < n) g[j] = gtf[c * S + s + j];
                    }
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        if (g[j] >= 0.5f) gb[j] |= 1u << c;
                }
            }
        } else if (gtb) {                                                       // raw mask bytes: fundus_map_mask / polyp_map_mask (datasets2d.py:90-142, 200-223)
            unsigned m0[4] = {0, 0, 0, 0}, m1[4] = {0, 0, 0, 0};
            const bool two = t.gt_map != 3;
            if (VEC) {
                const uint32_t l0 = *reinterpret_cast<const uint32_t*>(gtb + s), l1 = two ? *reinterpret_cast<const uint32_t*>(gtb + S + s) : 0u;
                m0[0] = l0 & 255; m0[1] = (l0 >> 8) & 255; m0[2] = (l0 >> 16) & 255; m0[3] = l0 >> 24;
                m1[0] = l1 & 255; m1[1] = (l1 >> 8) & 255; m1[2] = (l1 >> 16) & 255; m1[3] = l1 >> 24;
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (j < n) { m0[j] = gtb[s + j]; if (two) m1[j] = gtb[S + s + j]; }
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const unsigned disc = m0[j] >= 1, cup = m1[j] >= 1;             // polyp: `disc` is the polyp class, m1 stays 0
                gb[j] = ((t.gt_map == 2 ? disc & (cup ^ 1u) : disc) << 1) | (cup << 2);
            }
        }
        if (counts) {
#pragma unroll
            for (int c = 1; c < MAXC; ++c) {
                if (c < C) {
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const int on = (pb[j] >> c) & 1, hit = (gb[j] >> c) & 1;
                        ci[c - 1] += on & hit; cp[c - 1] += on; cg[c - 1] += hit;
                    }
                }
            }
        }
        if (ext) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (pb[j] & 2u) { lo[0] = min(lo[0], yj[j]); hi[0] = max(hi[0], yj[j]); }
                if (pb[j] & 4u) { lo[1] = min(lo[1], yj[j]); hi[1] = max(hi[1], yj[j]); }
                if (gb[j] & 2u) { lo[2] = min(lo[2], yj[j]); hi[2] = max(hi[2], yj[j]); }
                if (gb[j] & 4u) { lo[3] = min(lo[3], yj[j]); hi[3] = max(hi[3], yj[j]); }
            }
        }
        if (labels) {                                                           // nhot_to_values: ascending, a later class wins; 0 where none is on
            unsigned lab[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                int val = 0;
#pragma unroll
                for (int c = 0; c < MAXC; ++c)
                    if (c < C && ((pb[j] >> c) & 1)) val = vals[c];
                lab[j] = (unsigned)(uint8_t)val;
            }
            if (VEC) {
                *reinterpret_cast<uint32_t*>(labels + b * S + s) = lab[0] | (lab[1] << 8) | (lab[2] << 16) | (lab[3] << 24);
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (j < n) labels[b * S + s + j] = (uint8_t)lab[j];
            }
        }
        if (hard) {
            float* hb = hard + b * C * S + s;
#pragma unroll
            for (int c = 0; c < MAXC; ++c) {
                if (c < C) {
                    if (VEC) {
                        *reinterpret_cast<float4*>(hb + c * S) = make_float4((pb[0] >> c) & 1 ? 1.0f : 0.0f, (pb[1] >> c) & 1 ? 1.0f : 0.0f,
                                                                             (pb[2] >> c) & 1 ? 1.0f : 0.0f, (pb[3] >> c) & 1 ? 1.0f : 0.0f);
                    } else {
#pragma unroll
                        for (int j = 0; j < 4; ++j)
                            if (j < n) hb[c * S + j] = (pb[j] >> c) & 1 ? 1.0f : 0.0f;
                    }
                }
            }
        }
    }
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if (counts) {                                                               // wave -> LDS -> one atomic add per counter per workgroup
#pragma unroll
        for (int c = 0; c < MAXC - 1; ++c) {
            if (c < C - 1) {
                const int a = wave_sum_int(ci[c]), p = wave_sum_int(cp[c]), h = wave_sum_int(cg[c]);
                if (lane == 0) { red[wave][3 * c] = a; red[wave][3 * c + 1] = p; red[wave][3 * c + 2] = h; }
            }
        }
    }
    if (ext) {                                                                  // wave -> LDS -> one atomicMin / atomicMax per extent per workgroup
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int l = wave_min_int(lo[k]), h = wave_max_int(hi[k]);
            if (lane == 0) { redx[wave][2 * k] = l; redx[wave][2 * k + 1] = h; }
        }
    }
    __syncthreads();
    if (counts && (int)threadIdx.x < 3 * (C - 1)) {
        int tot = 0;
#pragma unroll
        for (int w = 0; w < CT_WAVES; ++w) tot += red[w][threadIdx.x];
        if (tot) atomicAdd(counts + b * 3 * (C - 1) + threadIdx.x, tot);
    }
    if (ext && threadIdx.x < 8) {                                               // ext[b][which][class][lowest, highest]: even entries are minima, odd ones maxima
        const bool is_max = threadIdx.x & 1;
        int e = redx[0][threadIdx.x];
#pragma unroll
        for (int w = 1; w < CT_WAVES; ++w) e = is_max ? max(e, redx[w][threadIdx.x]) : min(e, redx[w][threadIdx.x]);
        if (is_max) { if (e >= 0) atomicMax(ext + b * 8 + threadIdx.x, e); }
        else if (e < q.H) atomicMin(ext + b * 8 + threadIdx.x, e);
    }
}

}  // namespace segx

using namespace segx;
#define SEGX_STREAM hipStream_t stream = (hipStream_t)stream_

static inline int64_t edt_bins(int D, int H, int W) { return (int64_t)(D - 1) * (D - 1) + (int64_t)(H - 1) * (H - 1) + (int64_t)(W - 1) * (W - 1) + 1; }

extern "C" int segx_surface_border(const float* mask, uint8_t* border, int64_t planes, int D, int H, int W, int nd, void* stream_) {
    SEGX_STREAM; SEGX_REQUIRE(mask && border, "segx_surface_border: null pointer");
    SEGX_REQUIRE(planes > 0 && D > 0 && H > 0 && W > 0, "segx_surface_border: planes, D, H and W must be positive");
    SEGX_REQUIRE(nd == 2 || nd == 3, "segx_surface_border: nd is 2 or 3, not %d", nd);
    const int64_t total = planes * D * H * W;
    hipLaunchKernelGGL(surface_border_kernel, dim3((unsigned)i64min(65536, (total + 255) / 256)), dim3(256), 0, stream, mask, border, planes, D, H, W, nd);
    return check_launch("segx_surface_border");
}

extern "C" int segx_edt_sq(const uint8_t* border, int32_t* d2, int64_t planes, int D, int H, int W, void* stream_) {
    SEGX_STREAM; SEGX_REQUIRE(border && d2, "segx_edt_sq: null pointer");
    SEGX_REQUIRE(planes > 0 && D > 0 && H > 0 && W > 0, "segx_edt_sq: planes, D, H and W must be positive");
    SEGX_REQUIRE(D <= EDT_MAX && H <= EDT_MAX && W <= EDT_MAX, "segx_edt_sq: extents %d x %d x %d above the cap of %d per axis", D, H, W, EDT_MAX);
    const int64_t rows = planes * D * H;
    hipLaunchKernelGGL(edt_row_kernel, dim3((unsigned)i64min(65536, (rows + 3) / 4)), dim3(256), 0, stream, border, d2, rows, W);
    if (H > 1) {
        const int64_t items = planes * D * ((W + EDT_SLAB - 1) / EDT_SLAB);
        hipLaunchKernelGGL(edt_axis_kernel, dim3((unsigned)i64min(1 << 20, items)), dim3(256), 0, stream, d2, planes * D, H, (int64_t)W);
    }
    if (D > 1) {
        const int64_t inner = (int64_t)H * W, items = planes * ((inner + EDT_SLAB - 1) / EDT_SLAB);
        hipLaunchKernelGGL(edt_axis_kernel, dim3((unsigned)i64min(1 << 20, items)), dim3(256), 0, stream, d2, planes, D, inner);
    }
    return check_launch("segx_edt_sq");
}

extern "C" int segx_surface_hist(const uint8_t* border_from, const int32_t* d2_to, int32_t* hist, int64_t planes, int D, int H, int W, int nbins, void* stream_) {
    SEGX_STREAM; SEGX_REQUIRE(border_from && d2_to && hist, "segx_surface_hist: null pointer");
    SEGX_REQUIRE(planes > 0 && planes <= 65535 && D > 0 && H > 0 && W > 0, "segx_surface_hist: 1 <= planes <= 65535, D, H and W positive");
    SEGX_REQUIRE(D <= EDT_MAX && H <= EDT_MAX && W <= EDT_MAX, "segx_surface_hist: extents %d x %d x %d above the cap of %d per axis", D, H, W, EDT_MAX);
    SEGX_REQUIRE(nbins >= edt_bins(D, H, W), "segx_surface_hist: nbins %d below (D-1)^2 + (H-1)^2 + (W-1)^2 + 1 = %lld", nbins, (long long)edt_bins(D, H, W));
    const int64_t S = (int64_t)D * H * W;
    hipLaunchKernelGGL(surface_hist_kernel, dim3((unsigned)i64max(1, i64min(1024, (S + 4095) / 4096)), (unsigned)planes), dim3(256), 0, stream, border_from, d2_to,
                       hist, S, nbins);
    return check_launch("segx_surface_hist");
}

extern "C" int segx_brats_case_tail(const float* soft, const float* hard, const int32_t* gt, int32_t* counts, uint8_t* labels, int64_t S, void* stream_) {
    SEGX_STREAM; SEGX_REQUIRE(soft && hard, "segx_brats_case_tail: null soft or hard");
    SEGX_REQUIRE(counts || labels, "segx_brats_case_tail: neither counts nor labels asked for");
    SEGX_REQUIRE(!counts || gt, "segx_brats_case_tail: counts need the ground truth");
    SEGX_REQUIRE(S > 0 && S < ((int64_t)1 << 31), "segx_brats_case_tail: S = %lld is not in 1 .. 2^31 - 1", (long long)S);
    if (counts) hipLaunchKernelGGL(case_tail_init_kernel, dim3(1), dim3(64), 0, stream, counts);
    // a plane starts c * S floats into its tensor: 16-byte loads are legal only when S % 4 == 0 (and the bases are aligned)
    const uintptr_t a16 = (uintptr_t)soft | (uintptr_t)hard | (counts ? (uintptr_t)gt : 0);
    const bool vec = S % 4 == 0 && a16 % 16 == 0 && (uintptr_t)labels % 4 == 0;
    const dim3 grid((unsigned)i64min(SEGX_CASE_TAIL_MAX_BLOCKS, ((S + 3) / 4 + CT_THREADS - 1) / CT_THREADS));
    if (vec) hipLaunchKernelGGL(brats_case_tail_kernel<true>, grid, dim3(CT_THREADS), 0, stream, soft, hard, gt, counts, labels, S);
    else hipLaunchKernelGGL(brats_case_tail_kernel<false>, grid, dim3(CT_THREADS), 0, stream, soft, hard, gt, counts, labels, S);
    return check_launch("segx_brats_case_tail");
}

extern "C" int segx_index_onehot(const void* labels, int label_bytes, float* out, int64_t B, int C, int64_t S, void* stream_) {
    SEGX_STREAM; SEGX_REQUIRE(labels && out, "segx_index_onehot: null pointer");
    SEGX_REQUIRE(label_bytes == 1 || label_bytes == 4, "segx_index_onehot: labels are uint8 (1) or int32 (4), not %d bytes", label_bytes);
    SEGX_REQUIRE(B > 0 && S > 0, "segx_index_onehot: B and S must be positive");
    SEGX_REQUIRE(C >= 1 && C <= SEGX_MAX_CLASSES, "segx_index_onehot: C = %d is not in 1 .. %d", C, SEGX_MAX_CLASSES);
    const dim3 grid((unsigned)i64min(65536, (B * S + 255) / 256));
    if (label_bytes == 1) hipLaunchKernelGGL(index_onehot_kernel<1>, grid, dim3(256), 0, stream, labels, out, B, C, S);
    else hipLaunchKernelGGL(index_onehot_kernel<4>, grid, dim3(256), 0, stream, labels, out, B, C, S);
    return check_launch("segx_index_onehot");
}

extern "C" int segx_onehot_colormap(const float* nhot, const uint8_t* colormap, uint8_t* out, int64_t B, int C, int64_t S, void* stream_) {
    SEGX_STREAM; SEGX_REQUIRE(nhot && out, "segx_onehot_colormap: null nhot or out");
    SEGX_REQUIRE(B > 0 && S > 0, "segx_onehot_colormap: B and S must be positive");
    SEGX_REQUIRE(C >= 1 && C <= SEGX_MAX_CLASSES, "segx_onehot_colormap: C = %d is not in 1 .. %d", C, SEGX_MAX_CLASSES);
    hipLaunchKernelGGL(onehot_colormap_kernel, dim3((unsigned)i64min(65536, (B * S + 255) / 256)), dim3(256), 0, stream, nhot, colormap, out, B, C, S);
    return check_launch("segx_onehot_colormap");
}

template <int MAXC>
static void launch_onehot_case_tail(bool vec, dim3 grid, hipStream_t stream, const float* soft, const uint8_t* gt, const uint8_t* colormap, int32_t* counts,
                                    uint8_t* labels, uint8_t* rgb, int C, int64_t S, float T) {
    if (vec) hipLaunchKernelGGL((onehot_case_tail_kernel<MAXC, true>), grid, dim3(CT_THREADS), 0, stream, soft, gt, colormap, counts, labels, rgb, C, S, T);
    else hipLaunchKernelGGL((onehot_case_tail_kernel<MAXC, false>), grid, dim3(CT_THREADS), 0, stream, soft, gt, colormap, counts, labels, rgb, C, S, T);
}

extern "C" int segx_onehot_case_tail(const float* soft, const uint8_t* gt, const uint8_t* colormap, int32_t* counts, uint8_t* labels, uint8_t* rgb, int B, int C,
                                     int64_t S, float T, void* stream_) {
    SEGX_STREAM; SEGX_REQUIRE(soft, "segx_onehot_case_tail: null soft");
    SEGX_REQUIRE(counts || labels || rgb, "segx_onehot_case_tail: none of counts, labels and rgb asked for");
    SEGX_REQUIRE(!counts || gt, "segx_onehot_case_tail: counts need the ground truth");
    SEGX_REQUIRE(!rgb || colormap, "segx_onehot_case_tail: rgb needs the colormap");
    SEGX_REQUIRE(B > 0 && B <= 65535, "segx_onehot_case_tail: B = %d is not in 1 .. 65535", B);
    SEGX_REQUIRE(C >= 2 && C <= SEGX_MAX_CLASSES, "segx_onehot_case_tail: C = %d is not in 2 .. %d", C, SEGX_MAX_CLASSES);
    SEGX_REQUIRE(S > 0 && S < ((int64_t)1 << 31), "segx_onehot_case_tail: S = %lld is not in 1 .. 2^31 - 1", (long long)S);
    if (counts) {
        const int n = B * 3 * (C - 1);
        hipLaunchKernelGGL(onehot_tail_init_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, counts, n);
    }
    // a plane starts (b * C + c) * S floats into soft, an image b * S bytes into gt / labels and 3 * b * S into rgb: wide accesses are legal only when S % 4 == 0
    const bool vec = S % 4 == 0 && (uintptr_t)soft % 16 == 0 && ((counts ? (uintptr_t)gt : 0) | (uintptr_t)labels | (uintptr_t)rgb) % 4 == 0;
    const dim3 grid((unsigned)i64min(SEGX_CASE_TAIL_MAX_BLOCKS, ((S + 3) / 4 + CT_THREADS - 1) / CT_THREADS), (unsigned)B);
    if (C <= 8) launch_onehot_case_tail<8>(vec, grid, stream, soft, gt, colormap, counts, labels, rgb, C, S, T);
    else launch_onehot_case_tail<SEGX_MAX_CLASSES>(vec, grid, stream, soft, gt, colormap, counts, labels, rgb, C, S, T);
    return check_launch("segx_onehot_case_tail");
}

template <int MAXC>
static void launch_nhot_case_tail(bool vec, dim3 grid, hipStream_t stream, const float* soft, const void* gt, const int32_t* values, int32_t* counts, int32_t* ext,
                                  uint8_t* labels, float* hard, InterpDims q, NhotTail t) {
    if (vec) hipLaunchKernelGGL((nhot_case_tail_kernel<MAXC, true>), grid, dim3(CT_THREADS), 0, stream, soft, gt, values, counts, ext, labels, hard, q, t);
    else hipLaunchKernelGGL((nhot_case_tail_kernel<MAXC, false>), grid, dim3(CT_THREADS), 0, stream, soft, gt, values, counts, ext, labels, hard, q, t);
}

extern "C" int segx_nhot_case_tail(const float* soft, const void* gt, int gt_map, int gt_channels, const int32_t* values, int32_t* counts, int32_t* ext,
                                   uint8_t* labels, float* hard, int B, int C, int h, int w, int H, int W, float T, void* stream_) {
    SEGX_STREAM; SEGX_REQUIRE(soft, "segx_nhot_case_tail: null soft");
    SEGX_REQUIRE(counts || ext || labels || hard, "segx_nhot_case_tail: none of counts, ext, labels and hard asked for");
    SEGX_REQUIRE(!counts || gt, "segx_nhot_case_tail: counts need the ground truth");
    SEGX_REQUIRE(!ext || gt, "segx_nhot_case_tail: the ground-truth extents need the ground truth");
    SEGX_REQUIRE(!labels || values, "segx_nhot_case_tail: labels need the value table");
    SEGX_REQUIRE(B > 0 && B <= 65535, "segx_nhot_case_tail: B = %d is not in 1 .. 65535", B);
    SEGX_REQUIRE(C >= 2 && C <= SEGX_MAX_CLASSES, "segx_nhot_case_tail: C = %d is not in 2 .. %d", C, SEGX_MAX_CLASSES);
    SEGX_REQUIRE(h > 0 && w > 0, "segx_nhot_case_tail: the source size %d x %d must be positive", h, w);
    SEGX_REQUIRE(H > 0 && W > 0 && (int64_t)H * W < ((int64_t)1 << 31), "segx_nhot_case_tail: H * W = %lld is not in 1 .. 2^31 - 1", (long long)H * W);
    SEGX_REQUIRE(gt_map >= 0 && gt_map <= 3, "segx_nhot_case_tail: gt_map %d is not 0 (n-hot), 1 / 2 (fundus, exclusive) or 3 (polyp)", gt_map);
    if (gt && (gt_map == 1 || gt_map == 2))
        SEGX_REQUIRE(C == 3 && gt_channels >= 2, "segx_nhot_case_tail: a fundus mask has >= 2 channels and maps to 3 classes, not %d and %d", gt_channels, C);
    if (gt && gt_map == 3)
        SEGX_REQUIRE(C == 2 && gt_channels >= 1, "segx_nhot_case_tail: a polyp mask has >= 1 channel and maps to 2 classes, not %d and %d", gt_channels, C);
    if (counts || ext) {
        const int ncounts = counts ? B * 3 * (C - 1) : 0, npairs = ext ? B * 4 : 0, n = ncounts > npairs ? ncounts : npairs;
        hipLaunchKernelGGL(nhot_tail_init_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, counts, ncounts, ext, npairs, H);
    }
    const int64_t S = (int64_t)H * W;
    NhotTail t; t.C = C; t.Cm = gt_map == 0 ? C : gt_channels; t.gt_map = gt_map; t.same = h == H && w == W; t.T = T;
    // a plane starts a multiple of S elements into its tensor: wide accesses are legal only when S % 4 == 0.  soft is read wide only on the no-resample path.
    const uintptr_t a16 = (t.same ? (uintptr_t)soft : 0) | (uintptr_t)hard | (gt && gt_map == 0 ? (uintptr_t)gt : 0);
    const uintptr_t a4 = (uintptr_t)labels | (gt && gt_map != 0 ? (uintptr_t)gt : 0);
    const bool vec = S % 4 == 0 && a16 % 16 == 0 && a4 % 4 == 0;
    const dim3 grid((unsigned)i64min(SEGX_CASE_TAIL_MAX_BLOCKS, ((S + 3) / 4 + CT_THREADS - 1) / CT_THREADS), (unsigned)B);
    const InterpDims q = make_dims(1, h, w, 1, H, W);
    if (C <= 8) launch_nhot_case_tail<8>(vec, grid, stream, soft, gt, values, counts, ext, labels, hard, q, t);
    else launch_nhot_case_tail<SEGX_MAX_CLASSES>(vec, grid, stream, soft, gt, values, counts, ext, labels, hard, q, t);
    return check_launch("segx_nhot_case_tail");
}
