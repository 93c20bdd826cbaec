// infer.hip -- sliding-window evaluation path: test_single_batch (test_util2d.py:153-227),
// test_single_case (test_util3d.py:93-184), harden_segmap2d/3d (datasets2d.py:178-196, datasets3d.py:92-111),
// make_brats_pred_consistent (datasets3d.py:43-63), calc_dice (test_util2d.py:233-240).
//
// All HBM-bound, one pass each: the per-window tail `F.interpolate(scores -> window) ; sigmoid ; preds_soft[window] += ; cnt += 1`
// is ONE kernel (the reference makes four full-size temporaries per window), and the per-image tail
// `preds_soft / cnt ; consistency ; >= 0.5 ; background = no other class` is another.
#include "resample.h"
#include "harden.h"

namespace segx {

struct Canvas { int CD, CH, CW, oz, oy, ox; };          // canvas spatial dims and the window's origin inside it

// probability one window contributes at its position (z, y, x): sigmoid of the score plane s[d][h][w] resampled to the window (window_accum_kernel and
// window_merge_kernel both call it: the same expression, hence the same bits)
__device__ __forceinline__ float window_prob(const float* __restrict__ s, const InterpDims& q, bool same, int z, int y, int x) {
    const float v = same ? s[((int64_t)z * q.h + y) * q.w + x] : interp_at(s, q, z, y, x);
    return 1.0f / (1.0f + expf(-v));
}

// acc[b][c][oz+z][oy+y][ox+x] += sigmoid(resample(scores[b][c]))(z, y, x);  cnt[b][oz+z][oy+y][ox+x] += 1.   One thread per
// window voxel (all classes), so a launch never touches a canvas cell twice; overlapping windows are separate launches.
__global__ __launch_bounds__(256) void window_accum_kernel(const float* __restrict__ scores, float* __restrict__ acc, float* __restrict__ cnt,
                                                           int B, int C, InterpDims q, Canvas cv) {
    const int64_t wsz = (int64_t)q.D * q.H * q.W, ssz = (int64_t)q.d * q.h * q.w, csz = (int64_t)cv.CD * cv.CH * cv.CW, total = (int64_t)B * wsz;
    const bool same = q.d == q.D && q.h == q.H && q.w == q.W;
    for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * 256) {
        const int b = (int)(idx / wsz); int64_t r = idx - (int64_t)b * wsz;
        const int z = (int)(r / ((int64_t)q.H * q.W)); r -= (int64_t)z * q.H * q.W;
        const int y = (int)(r / q.W), x = (int)(r - (int64_t)y * q.W);
        const int64_t cell = ((int64_t)(cv.oz + z) * cv.CH + (cv.oy + y)) * cv.CW + (cv.ox + x);
        for (int c = 0; c < C; ++c) {
            acc[((int64_t)b * C + c) * csz + cell] += window_prob(scores + ((int64_t)b * C + c) * ssz, q, same, z, y, x);
        }
        cnt[(int64_t)b * csz + cell] += 1.0f;
    }
}

// the mean of the covering windows' probabilities
__device__ __forceinline__ float mean_prob(float a, float n) { return a / n; }
// harden_cell<MAXC> (harden.h): one cell's C soft values -> the soft / hard planes; harden_kernel and window_merge_kernel both call it.

// soft = acc / cnt (cnt == NULL: acc already is the soft map), then harden_cell.  One thread per voxel.
template <int MAXC>
__global__ __launch_bounds__(256) void harden_kernel(const float* __restrict__ acc, const float* __restrict__ cnt, float* __restrict__ soft,
                                                     float* __restrict__ hard, int B, int C, int64_t S, int mode, float T) {
    const int64_t total = (int64_t)B * S;
    for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * 256) {
        const int64_t b = idx / S, s = idx - b * S;
        const float n = cnt ? cnt[idx] : 1.0f;
        float p[MAXC];
#pragma unroll
        for (int c = 0; c < MAXC; ++c) {
            p[c] = 0.0f;
            if (c < C) p[c] = cnt ? mean_prob(acc[(b * C + c) * S + s], n) : acc[(b * C + c) * S + s];
        }
        harden_cell<MAXC>(p, C, mode, T, soft ? soft + (b * C) * S + s : nullptr, hard + (b * C) * S + s, S);
    }
}

// ---- the whole sliding-window evaluation as gather -> network on stacked windows -> merge (two launches around the forwards, capturable) ----
// origins: int32 [nwin][3] = {oz, oy, ox} of each window in PADDED-canvas coordinates, in the order the eager loops visit the windows.
struct Sliding { int CD, CH, CW, pz, py, px, ID, IH, IW; };   // padded canvas, left pads, image (the un-padded region of the canvas)

// out[k * B + b][c] = the window crop of image[b][c] at origin k; canvas cells outside the image read 0 (the zero padding never exists in memory).  One thread per
// output element; every read is checked against the image, whatever the table holds.
__global__ __launch_bounds__(256) void window_gather_kernel(const float* __restrict__ image, const int* __restrict__ origins, float* __restrict__ out,
                                                            int nwin, int B, int C, int D, int H, int W, Sliding sl) {
    const int64_t wsz = (int64_t)D * H * W, total = (int64_t)nwin * B * C * wsz;
    for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * 256) {
        const int64_t pl = idx / wsz; int64_t r = idx - pl * wsz;            // pl = (k * B + b) * C + c
        const int z = (int)(r / ((int64_t)H * W)); r -= (int64_t)z * H * W;
        const int y = (int)(r / W), x = (int)(r - (int64_t)y * W);
        const int c = (int)(pl % C), kb = (int)(pl / C), b = kb % B, k = kb / B;
        const int iz = origins[3 * k] - sl.pz + z, iy = origins[3 * k + 1] - sl.py + y, ix = origins[3 * k + 2] - sl.px + x;      // image coordinates
        const bool in = (unsigned)iz < (unsigned)sl.ID && (unsigned)iy < (unsigned)sl.IH && (unsigned)ix < (unsigned)sl.IW;
        out[idx] = in ? image[((((int64_t)b * C + c) * sl.ID + iz) * sl.IH + iy) * sl.IW + ix] : 0.0f;
    }
}

// soft[b][c][cell] = (sum over the windows k covering the cell, ascending k, of window_prob(scores[k * B + b][c])) / (their count), then harden_cell: what
// nwin segx_window_accum passes over zeroed acc / cnt followed by segx_harden_segmap leave, restricted to the image (the un-padded region), without acc / cnt
// in memory.  One thread per image cell (all classes); the covering windows are found by a pass over the table (uniform loads: k is the same in every lane).
// MAXC as in harden_cell.  EXACT: the class count IS MAXC (the 2-, 3- and 4-class tasks): no predicate is left, the classes' loads of a window issue together.
template <int MAXC, bool EXACT>
__global__ __launch_bounds__(256) void window_merge_kernel(const float* __restrict__ scores, const int* __restrict__ origins, float* __restrict__ soft,
                                                           float* __restrict__ hard, int nwin, int B, int C_, InterpDims q, Sliding sl, int mode, float T) {
    const int C = EXACT ? MAXC : C_;
    const int64_t isz = (int64_t)sl.ID * sl.IH * sl.IW, ssz = (int64_t)q.d * q.h * q.w, total = (int64_t)B * isz;
    const bool same = q.d == q.D && q.h == q.H && q.w == q.W;
    for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * 256) {
        const int64_t b = idx / isz, cell = idx - b * isz; int64_t r = cell;
        const int z = (int)(r / ((int64_t)sl.IH * sl.IW)); r -= (int64_t)z * sl.IH * sl.IW;
        const int y = (int)(r / sl.IW), x = (int)(r - (int64_t)y * sl.IW);
        float p[MAXC], n = 0.0f;
#pragma unroll
        for (int c = 0; c < MAXC; ++c) p[c] = 0.0f;
        for (int k = 0; k < nwin; ++k) {
            const int wz = z + sl.pz - origins[3 * k], wy = y + sl.py - origins[3 * k + 1], wx = x + sl.px - origins[3 * k + 2];
            if ((unsigned)wz >= (unsigned)q.D || (unsigned)wy >= (unsigned)q.H || (unsigned)wx >= (unsigned)q.W) continue;
#pragma unroll
            for (int c = 0; c < MAXC; ++c)
                if (c < C) p[c] += window_prob(scores + (((int64_t)k * B + b) * C + c) * ssz, q, same, wz, wy, wx);
            n += 1.0f;
        }
#pragma unroll
        for (int c = 0; c < MAXC; ++c)
            if (c < C) p[c] = mean_prob(p[c], n);
        harden_cell<MAXC>(p, C, mode, T, soft + (b * C) * isz + cell, hard + (b * C) * isz + cell, isz);
    }
}

// ---- flip test-time augmentation: a view is a set of flipped image axes (bit 0 = the depth axis ID, bit 1 = IH, bit 2 = IW); views: int32 [V] masks ----
// the coordinate of the flipped image's cell i along an axis of extent n: the mirror when the view flips the axis.  Its own inverse.
__device__ __forceinline__ int view_coord(int i, int n, bool flip) { return flip ? n - 1 - i : i; }

// out[(v * nwin + k) * B + b][c] = the crop of window k from the zero-padded image FLIPPED along view v's axes (the flip is of the un-padded image, so pads and
// origins are the un-flipped geometry's); read from the un-flipped image through the mirrored coordinate: neither the flipped image nor its canvas exists.
// window_gather_kernel with one more digit in the index; the bounds check is against the image.
__global__ __launch_bounds__(256) void window_gather_views_kernel(const float* __restrict__ image, const int* __restrict__ origins, const int* __restrict__ views,
                                                                  float* __restrict__ out, int nwin, int V, int B, int C, int D, int H, int W, Sliding sl) {
    const int64_t wsz = (int64_t)D * H * W, total = (int64_t)V * nwin * B * C * wsz;
    for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * 256) {
        const int64_t pl = idx / wsz; int64_t r = idx - pl * wsz;            // pl = ((v * nwin + k) * B + b) * C + c
        const int z = (int)(r / ((int64_t)H * W)); r -= (int64_t)z * H * W;
        const int y = (int)(r / W), x = (int)(r - (int64_t)y * W);
        const int c = (int)(pl % C), vkb = (int)(pl / C), b = vkb % B, vk = vkb / B, k = vk % nwin, m = views[vk / nwin];
        const int fz = origins[3 * k] - sl.pz + z, fy = origins[3 * k + 1] - sl.py + y, fx = origins[3 * k + 2] - sl.px + x;      // flipped-image coordinates
        const bool in = (unsigned)fz < (unsigned)sl.ID && (unsigned)fy < (unsigned)sl.IH && (unsigned)fx < (unsigned)sl.IW;
        const int iz = view_coord(fz, sl.ID, m & 1), iy = view_coord(fy, sl.IH, m & 2), ix = view_coord(fx, sl.IW, m & 4);      // inside the image iff (fz, fy, fx) is
        out[idx] = in ? image[((((int64_t)b * C + c) * sl.ID + iz) * sl.IH + iy) * sl.IW + ix] : 0.0f;
    }
}

// soft[b][c][cell] = (((soft_0 + soft_1) + soft_2) + ...) / V, then harden_cell, where soft_v[cell] is what window_merge_kernel writes as soft for the scores of view v
// (rows (v * nwin + k) * B + b) at the MIRRORED cell, i.e. view v's soft map flipped back: the loop of window_merge_kernel (ascending k, window_prob, mean_prob and,
// in mode 1, the consistency rule its harden_cell applies before it writes soft) once per view, in the views' order, into a register accumulator per class.
// A view's term is a quotient and the accumulation adds quotients: no product feeds an add, so there is nothing a contraction could fuse.
template <int MAXC, bool EXACT>
__global__ __launch_bounds__(256) void window_merge_views_kernel(const float* __restrict__ scores, const int* __restrict__ origins, const int* __restrict__ views,
                                                                 float* __restrict__ soft, float* __restrict__ hard, int nwin, int V, int B, int C_, InterpDims q,
                                                                 Sliding sl, int mode, float T) {
    const int C = EXACT ? MAXC : C_;
    const int64_t isz = (int64_t)sl.ID * sl.IH * sl.IW, ssz = (int64_t)q.d * q.h * q.w, total = (int64_t)B * isz;
    const bool same = q.d == q.D && q.h == q.H && q.w == q.W;
    const float fV = (float)V;
    for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * 256) {
        const int64_t b = idx / isz, cell = idx - b * isz; int64_t r = cell;
        const int z = (int)(r / ((int64_t)sl.IH * sl.IW)); r -= (int64_t)z * sl.IH * sl.IW;
        const int y = (int)(r / sl.IW), x = (int)(r - (int64_t)y * sl.IW);
        float a[MAXC];
#pragma unroll
        for (int c = 0; c < MAXC; ++c) a[c] = 0.0f;
        for (int v = 0; v < V; ++v) {
            const int m = views[v];                                           // uniform: v is the same in every lane
            const int fz = view_coord(z, sl.ID, m & 1) + sl.pz, fy = view_coord(y, sl.IH, m & 2) + sl.py, fx = view_coord(x, sl.IW, m & 4) + sl.px;
            float p[MAXC], n = 0.0f;
#pragma unroll
            for (int c = 0; c < MAXC; ++c) p[c] = 0.0f;
            for (int k = 0; k < nwin; ++k) {
                const int wz = fz - origins[3 * k], wy = fy - origins[3 * k + 1], wx = fx - origins[3 * k + 2];
                if ((unsigned)wz >= (unsigned)q.D || (unsigned)wy >= (unsigned)q.H || (unsigned)wx >= (unsigned)q.W) continue;
#pragma unroll
                for (int c = 0; c < MAXC; ++c)
                    if (c < C) p[c] += window_prob(scores + ((((int64_t)v * nwin + k) * B + b) * C + c) * ssz, q, same, wz, wy, wx);
                n += 1.0f;
            }
#pragma unroll
            for (int c = 0; c < MAXC; ++c)
                if (c < C) p[c] = mean_prob(p[c], n);
            if constexpr (MAXC >= 4) {
                if (mode == 1) {                                              // the soft map of a view is the consistent one, as harden_cell writes it (C == 4)
                    const float et = p[1], wt = p[2], tc = p[3];
                    p[2] = fmaxf(fmaxf(et, wt), tc);
                    p[3] = fmaxf(et, tc);
                }
            }
#pragma unroll
            for (int c = 0; c < MAXC; ++c)
                if (c < C) a[c] = v == 0 ? p[c] : a[c] + p[c];                // the sum starts AT soft_0
        }
#pragma unroll
        for (int c = 0; c < MAXC; ++c)
            if (c < C) a[c] = a[c] / fV;
        harden_cell<MAXC>(a, C, mode, T, soft + (b * C) * isz + cell, hard + (b * C) * isz + cell, isz);
    }
}

// per (plane, chunk): sum pred*gt, sum pred^2, sum gt^2  ->  part[chunk][plane][3]  (summed over chunks by segx_colsum)
__global__ __launch_bounds__(256) void dice_sums_kernel(const float* __restrict__ pred, const float* __restrict__ gt, float* __restrict__ part,
                                                        int64_t S) {
    __shared__ float red[4];
    const int plane = blockIdx.y, chunk = blockIdx.x, planes = gridDim.y;
    const float* p = pred + (int64_t)plane * S; const float* g = gt + (int64_t)plane * S;
    float a = 0.f, b = 0.f, c = 0.f;
    for (int64_t s = (int64_t)chunk * 256 + threadIdx.x; s < S; s += (int64_t)gridDim.x * 256) {
        const float pv = p[s], gv = g[s];
        a += pv * gv; b += pv * pv; c += gv * gv;
    }
    a = block_sum<4>(a, red); b = block_sum<4>(b, red); c = block_sum<4>(c, red);
    if (threadIdx.x == 0) { float* o = part + ((int64_t)chunk * planes + plane) * 3; o[0] = a; o[1] = b; o[2] = c; }
}

}  // namespace segx

using namespace segx;
#define SEGX_STREAM hipStream_t stream = (hipStream_t)stream_

/* scores [B, C, d, h, w] -> window [D, H, W] at origin (oz, oy, ox) of the canvas acc [B, C, CD, CH, CW], cnt [B, CD, CH, CW];
 * geom (int32[12]) = {d, h, w, D, H, W, CD, CH, CW, oz, oy, ox};  2-D: d = D = CD = 1, oz = 0 */
extern "C" int segx_window_accum(const float* scores, float* acc, float* cnt, int B, int C, const int* geom, void* stream_) {
    SEGX_STREAM; SEGX_REQUIRE(scores && acc && cnt && geom && B > 0 && C > 0, "segx_window_accum: bad args");
    const InterpDims q = make_dims(geom[0], geom[1], geom[2], geom[3], geom[4], geom[5]);
    const Canvas cv{geom[6], geom[7], geom[8], geom[9], geom[10], geom[11]};
    SEGX_REQUIRE(q.d > 0 && q.h > 0 && q.w > 0 && q.D > 0 && q.H > 0 && q.W > 0 && cv.oz >= 0 && cv.oy >= 0 && cv.ox >= 0 &&
                 cv.oz + q.D <= cv.CD && cv.oy + q.H <= cv.CH && cv.ox + q.W <= cv.CW, "segx_window_accum: window outside the canvas");
    const int64_t total = (int64_t)B * q.D * q.H * q.W;
    hipLaunchKernelGGL(window_accum_kernel, dim3((unsigned)i64min(65536, (total + 255) / 256)), dim3(256), 0, stream, scores, acc, cnt, B, C, q, cv);
    return check_launch("segx_window_accum");
}
/* mode 0: n-hot harden (harden_segmap2d/3d); mode 1: BraTS (make_brats_pred_consistent(is_conservative=False) then harden, C == 4).
 * cnt may be NULL (acc is already a probability map); soft may be NULL. */
extern "C" int segx_harden_segmap(const float* acc, const float* cnt, float* soft, float* hard, int B, int C, int64_t S, int mode, float T,
                                  void* stream_) {
    SEGX_STREAM; SEGX_REQUIRE(acc && hard && B > 0 && C >= 2 && C <= SEGX_MAX_CLASSES && S > 0 && (mode == 0 || (mode == 1 && C == 4)), "segx_harden_segmap: bad args");
    const int64_t total = (int64_t)B * S;
    const dim3 grid((unsigned)i64min(65536, (total + 255) / 256));
    if (C <= 8) hipLaunchKernelGGL(harden_kernel<8>, grid, dim3(256), 0, stream, acc, cnt, soft, hard, B, C, S, mode, T);
    else hipLaunchKernelGGL(harden_kernel<SEGX_MAX_CLASSES>, grid, dim3(256), 0, stream, acc, cnt, soft, hard, B, C, S, mode, T);
    return check_launch("segx_harden_segmap");
}
// every window of the host copy of the table inside the padded canvas, and the image inside it at the left pads
static bool sliding_ok(const int* o, int nwin, int D, int H, int W, const Sliding& sl) {
    if (sl.CD <= 0 || sl.CH <= 0 || sl.CW <= 0 || sl.ID <= 0 || sl.IH <= 0 || sl.IW <= 0 || sl.pz < 0 || sl.py < 0 || sl.px < 0 ||
        sl.pz + sl.ID > sl.CD || sl.py + sl.IH > sl.CH || sl.px + sl.IW > sl.CW) return false;
    for (int k = 0; k < nwin; ++k)
        if (o[3 * k] < 0 || o[3 * k + 1] < 0 || o[3 * k + 2] < 0 || o[3 * k] + D > sl.CD || o[3 * k + 1] + H > sl.CH || o[3 * k + 2] + W > sl.CW) return false;
    return true;
}
/* image [B, C, ID, IH, IW] -> out [nwin * B, C, D, H, W] (window-major, then image);  origins: device int32 [nwin][3], origins_host: the same table in host
 * memory (the refusals are decided on it);  geom (int32[12]) = {ID, IH, IW (image), pz, py, px (left pads), D, H, W (window), CD, CH, CW (padded canvas)} */
extern "C" int segx_window_gather(const float* image, const int* origins, const int* origins_host, float* out, int nwin, int B, int C, const int* geom,
                                  void* stream_) {
    SEGX_STREAM; SEGX_REQUIRE(image && origins && origins_host && out && geom, "segx_window_gather: null pointer");
    SEGX_REQUIRE(nwin > 0 && B > 0 && C > 0, "segx_window_gather: nwin, B and C must be positive");
    const Sliding sl{geom[9], geom[10], geom[11], geom[3], geom[4], geom[5], geom[0], geom[1], geom[2]};
    const int D = geom[6], H = geom[7], W = geom[8];
    SEGX_REQUIRE(D > 0 && H > 0 && W > 0, "segx_window_gather: bad window size");
    SEGX_REQUIRE(sliding_ok(origins_host, nwin, D, H, W, sl), "segx_window_gather: window outside the padded canvas");
    const int64_t total = (int64_t)nwin * B * C * D * H * W;
    hipLaunchKernelGGL(window_gather_kernel, dim3((unsigned)i64min(65536, (total + 255) / 256)), dim3(256), 0, stream, image, origins, out, nwin, B, C, D, H, W, sl);
    return check_launch("segx_window_gather");
}
/* scores [nwin * B, C, d, h, w] -> soft, hard [B, C, ID, IH, IW] (hard as 0/1 floats);  origins / origins_host as segx_window_gather;
 * geom (int32[15]) = {d, h, w (scores), D, H, W (window), CD, CH, CW (padded canvas), pz, py, px (left pads), ID, IH, IW (image)};  mode, T as segx_harden_segmap */
extern "C" int segx_window_merge(const float* scores, const int* origins, const int* origins_host, float* soft, float* hard, int nwin, int B, int C,
                                 const int* geom, int mode, float T, void* stream_) {
    SEGX_STREAM; SEGX_REQUIRE(scores && origins && origins_host && soft && hard && geom, "segx_window_merge: null pointer");
    SEGX_REQUIRE(nwin > 0 && B > 0 && C >= 2 && C <= SEGX_MAX_CLASSES, "segx_window_merge: nwin and B must be positive, 2 <= C <= %d", SEGX_MAX_CLASSES);
    SEGX_REQUIRE(mode == 0 || (mode == 1 && C == 4), "segx_window_merge: mode is 0, or 1 with C == 4");
    SEGX_REQUIRE(geom[0] > 0 && geom[1] > 0 && geom[2] > 0 && geom[3] > 0 && geom[4] > 0 && geom[5] > 0, "segx_window_merge: bad scores / window size");
    const InterpDims q = make_dims(geom[0], geom[1], geom[2], geom[3], geom[4], geom[5]);
    const Sliding sl{geom[6], geom[7], geom[8], geom[9], geom[10], geom[11], geom[12], geom[13], geom[14]};
    SEGX_REQUIRE(sliding_ok(origins_host, nwin, q.D, q.H, q.W, sl), "segx_window_merge: window outside the padded canvas");
    const int64_t total = (int64_t)B * sl.ID * sl.IH * sl.IW;
    const dim3 grid((unsigned)i64min(65536, (total + 255) / 256));
    const dim3 block(256);
#define SEGX_MERGE(MAXC, EXACT) hipLaunchKernelGGL((window_merge_kernel<MAXC, EXACT>), grid, block, 0, stream, scores, origins, soft, hard, nwin, B, C, q, sl, mode, T)
    if (C == 2) SEGX_MERGE(2, true);                       // polyp
    else if (C == 3) SEGX_MERGE(3, true);                  // fundus
    else if (C == 4) SEGX_MERGE(4, true);                  // BraTS
    else if (C <= 8) SEGX_MERGE(8, false);
    else SEGX_MERGE(SEGX_MAX_CLASSES, false);
#undef SEGX_MERGE
    return check_launch("segx_window_merge");
}
// the host copy of the view table: 1..SEGX_MAX_VIEWS masks of the three axis bits, no mask twice, no bit of an axis the call does not have (image, window and canvas
// extent all 1: the depth axis of a 2-D call)
static bool views_ok(const int* m, int V, int D, int H, int W, const Sliding& sl) {
    if (V < 1 || V > SEGX_MAX_VIEWS) return false;
    const int absent = (D == 1 && sl.CD == 1 && sl.ID == 1 ? 1 : 0) | (H == 1 && sl.CH == 1 && sl.IH == 1 ? 2 : 0) | (W == 1 && sl.CW == 1 && sl.IW == 1 ? 4 : 0);
    for (int v = 0; v < V; ++v) {
        if (m[v] < 0 || m[v] > 7 || (m[v] & absent)) return false;
        for (int u = 0; u < v; ++u)
            if (m[u] == m[v]) return false;
    }
    return true;
}
/* segx_window_gather for V flipped views in one launch: out [V * nwin * B, C, D, H, W] (view-major, then window, then image);  views: device int32 [V] flip masks
 * (bit 0 = ID axis, bit 1 = IH, bit 2 = IW), views_host: the same in host memory (the refusals are decided on it);  the rest as segx_window_gather */
extern "C" int segx_window_gather_views(const float* image, const int* origins, const int* origins_host, const int* views, const int* views_host, float* out,
                                        int nwin, int V, int B, int C, const int* geom, void* stream_) {
    SEGX_STREAM; SEGX_REQUIRE(image && origins && origins_host && views && views_host && out && geom, "segx_window_gather_views: null pointer");
    SEGX_REQUIRE(nwin > 0 && B > 0 && C > 0, "segx_window_gather_views: nwin, B and C must be positive");
    const Sliding sl{geom[9], geom[10], geom[11], geom[3], geom[4], geom[5], geom[0], geom[1], geom[2]};
    const int D = geom[6], H = geom[7], W = geom[8];
    SEGX_REQUIRE(D > 0 && H > 0 && W > 0, "segx_window_gather_views: bad window size");
    SEGX_REQUIRE(sliding_ok(origins_host, nwin, D, H, W, sl), "segx_window_gather_views: window outside the padded canvas");
    SEGX_REQUIRE(views_ok(views_host, V, D, H, W, sl), "segx_window_gather_views: 1..%d distinct views, each a mask of the call's spatial axes", SEGX_MAX_VIEWS);
    const int64_t total = (int64_t)V * nwin * B * C * D * H * W;
    hipLaunchKernelGGL(window_gather_views_kernel, dim3((unsigned)i64min(65536, (total + 255) / 256)), dim3(256), 0, stream, image, origins, views, out, nwin, V, B, C,
                       D, H, W, sl);
    return check_launch("segx_window_gather_views");
}
/* segx_window_merge over V views: scores [V * nwin * B, C, d, h, w] (segx_window_gather_views' layout) -> soft, hard [B, C, ID, IH, IW];  views / views_host as
 * segx_window_gather_views;  the rest as segx_window_merge */
extern "C" int segx_window_merge_views(const float* scores, const int* origins, const int* origins_host, const int* views, const int* views_host, float* soft,
                                       float* hard, int nwin, int V, int B, int C, const int* geom, int mode, float T, void* stream_) {
    SEGX_STREAM; SEGX_REQUIRE(scores && origins && origins_host && views && views_host && soft && hard && geom, "segx_window_merge_views: null pointer");
    SEGX_REQUIRE(nwin > 0 && B > 0 && C >= 2 && C <= SEGX_MAX_CLASSES, "segx_window_merge_views: nwin and B must be positive, 2 <= C <= %d", SEGX_MAX_CLASSES);
    SEGX_REQUIRE(mode == 0 || (mode == 1 && C == 4), "segx_window_merge_views: mode is 0, or 1 with C == 4");
    SEGX_REQUIRE(geom[0] > 0 && geom[1] > 0 && geom[2] > 0 && geom[3] > 0 && geom[4] > 0 && geom[5] > 0, "segx_window_merge_views: bad scores / window size");
    const InterpDims q = make_dims(geom[0], geom[1], geom[2], geom[3], geom[4], geom[5]);
    const Sliding sl{geom[6], geom[7], geom[8], geom[9], geom[10], geom[11], geom[12], geom[13], geom[14]};
    SEGX_REQUIRE(sliding_ok(origins_host, nwin, q.D, q.H, q.W, sl), "segx_window_merge_views: window outside the padded canvas");
    SEGX_REQUIRE(views_ok(views_host, V, q.D, q.H, q.W, sl), "segx_window_merge_views: 1..%d distinct views, each a mask of the call's spatial axes", SEGX_MAX_VIEWS);
    const int64_t total = (int64_t)B * sl.ID * sl.IH * sl.IW;
    const dim3 grid((unsigned)i64min(65536, (total + 255) / 256));
    const dim3 block(256);
#define SEGX_MERGE(MAXC, EXACT) \
    hipLaunchKernelGGL((window_merge_views_kernel<MAXC, EXACT>), grid, block, 0, stream, scores, origins, views, soft, hard, nwin, V, B, C, q, sl, mode, T)
    if (C == 2) SEGX_MERGE(2, true);
    else if (C == 3) SEGX_MERGE(3, true);
    else if (C == 4) SEGX_MERGE(4, true);
    else if (C <= 8) SEGX_MERGE(8, false);
    else SEGX_MERGE(SEGX_MAX_CLASSES, false);
#undef SEGX_MERGE
    return check_launch("segx_window_merge_views");
}
extern "C" int64_t segx_dice_ws_floats(int64_t planes, int64_t S) { return 3 * planes * i64max(1, i64min(64, (S + 4095) / 4096)); }
/* part: segx_dice_ws_floats(planes, S) floats laid out [chunks][planes][3]; sums[planes][3] = segx_colsum over the chunks */
extern "C" int segx_dice_sums(const float* pred, const float* gt, float* part, int64_t planes, int64_t S, void* stream_) {
    SEGX_STREAM; SEGX_REQUIRE(pred && gt && part && planes > 0 && planes <= 65535 && S > 0, "segx_dice_sums: bad args");
    const int chunks = (int)i64max(1, i64min(64, (S + 4095) / 4096));
    hipLaunchKernelGGL(dice_sums_kernel, dim3(chunks, (unsigned)planes), dim3(256), 0, stream, pred, gt, part, S);
    return check_launch("segx_dice_sums");
}
