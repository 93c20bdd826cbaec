// mbconv_mid.hip -- the CHANNEL-RESIDENT MIDDLE of a stride-1 MBConv block (efficientnet/model.py:96-106 in training mode):
//     e --BatchNorm0 + swish--> e' --k x k depthwise 'same' convolution--> d --BatchNorm1 + swish (+ squeeze-excite pooling sums)--> d'
// for the blocks whose (sample, channel) plane is 1024 or 4096 floats and whose batch is <= 6: there ONE workgroup holds all planes of a channel in registers
// (what bn_act_{fwd,bwd}_res_kernel of backbone.hip already does for one BatchNorm), so both BatchNorm statistics, the convolution and -- backward -- all five
// channel sums and the complete filter gradient are formed on chip.  No workgroup waits for another one.
//   forward : read e; write d (saved for backward) and d'.                  3 passes over the expanded tensor, 1 launch  (three ops: 6 passes, 3 launches)
//   backward: read dy, d, e; write de.                                      4 passes, 1 launch                            (three ops: 10 passes, 4 launches)
// e' is never written: backward recomputes swish(BatchNorm0(e)) from e, which it reads anyway for BatchNorm0's gradient (saving e' would cost a write forward and
// a fourth read backward for one swish per element).
// The convolution runs out of LDS, one plane at a time: every thread writes ITS float4s of the plane (lane <-> element mapping of the resident BatchNorm kernels:
// float4 j = thread + NT * k), the workgroup meets, and every thread reads the K rows x 3 aligned float4 around each of its float4s.  Left and right borders read
// zero guard slots between the rows of the LDS image, rows above and below the plane are clamped reads + selects: H and W are free (H * W fixed per instantiation,
// W % 4 == 0).
// Forward results are bit-identical to bn_act_fwd_res_kernel -> dwconv_rows4_kernel -> bn_act_fwd_res_kernel<POOL>: same statistics order, same tap order
// (ky outer, kx inner, one fused multiply-add chain per output starting from zero; a padded tap adds w * 0).
#include "common.h"
#include <initializer_list>

namespace segx {

constexpr int MID_BMAX = 6;

// The plane's image in LDS: float4 (r, c4) at r * (W4 + 1) + 1 + c4; the slots r * (W4 + 1), r = 0 .. H, are zero guards (written once per workgroup), so the float4
// left of a row's first and right of its last one read as zeros.  H + 1 <= S4 + 1 guards whatever the shape.
template <int NT> __device__ __forceinline__ void mid_guards(f32x4* pl, int H, int W4) {
    for (int r = threadIdx.x; r <= H; r += NT) pl[r * (W4 + 1)] = f32x4{0.f, 0.f, 0.f, 0.f};
}
// the 12 floats around image position p (a float4 of row r) moved by dr rows: columns 4 c4 - 4 .. 4 c4 + 7 of row r + dr, zeros where that row is outside the plane
__device__ __forceinline__ void mid_window(float (&e)[12], const f32x4* pl, int p, int r, int dr, int H, int W4) {
    const bool rok = (unsigned)(r + dr) < (unsigned)H;
    const f32x4* q = pl + (rok ? p + dr * (W4 + 1) : p);
    const f32x4 a = q[-1], m = q[0], z = q[1];
    e[0] = rok ? a.x : 0.f; e[1] = rok ? a.y : 0.f; e[2] = rok ? a.z : 0.f; e[3] = rok ? a.w : 0.f;
    e[4] = rok ? m.x : 0.f; e[5] = rok ? m.y : 0.f; e[6] = rok ? m.z : 0.f; e[7] = rok ? m.w : 0.f;
    e[8] = rok ? z.x : 0.f; e[9] = rok ? z.y : 0.f; e[10] = rok ? z.z : 0.f; e[11] = rok ? z.w : 0.f;
}
// mean and sum of squares around the mean of the B live planes in v (idle planes are zeroed): bn_act_fwd_res_kernel's two passes over registers, same order
template <int NW, int KP>
__device__ __forceinline__ void mid_stats(f32x4 (&v)[MID_BMAX][KP], int B, float n, float* red, float& m, float& q) {
    float s = 0.f;
#pragma unroll
    for (int b = 0; b < MID_BMAX; ++b)
#pragma unroll
        for (int k = 0; k < KP; ++k) {
            if (b >= B) v[b][k] = f32x4{0.f, 0.f, 0.f, 0.f};
            s += (v[b][k].x + v[b][k].y) + (v[b][k].z + v[b][k].w);
        }
    m = block_sum<NW>(s, red) / n;
    q = 0.f;
#pragma unroll
    for (int b = 0; b < MID_BMAX; ++b)
#pragma unroll
        for (int k = 0; k < KP; ++k) {
            const float d0 = v[b][k].x - m, d1 = v[b][k].y - m, d2 = v[b][k].z - m, d3 = v[b][k].w - m;
            q += b < B ? (d0 * d0 + d1 * d1) + (d2 * d2 + d3 * d3) : 0.f;
        }
    q = block_sum<NW>(q, red);
}
__device__ __forceinline__ void mid_running(float* run_mean, float* run_var, int c, float momentum, float m, float q, float n) {
    if (run_mean) {
        run_mean[c] = (1.0f - momentum) * run_mean[c] + momentum * m;
        run_var[c] = (1.0f - momentum) * run_var[c] + momentum * (q / fmaxf(n - 1.0f, 1.0f));
    }
}

struct MidFwdArgs {
    const float* E; const float* w0; const float* b0; float* rm0; float* rv0; const float* Wdw; const float* w1; const float* b1; float* rm1; float* rv1;
    float* D; float* Y; float* psum; float* mean0; float* var0; float* mean1; float* var1;
    float mom0, eps0, mom1, eps1; int C, H, W4;
};
// grid = C workgroups of 256 threads; a plane is 256 * KP float4
template <int KP, int K>
__global__ __launch_bounds__(256) SEGX_MIN_WAVES_PER_SIMD(KP == 1 ? 4 : 2) void mbconv_mid_fwd_kernel(MidFwdArgs g, int B) {
    constexpr int NT = 256, P = K / 2, S4 = NT * KP;
    __shared__ float red[4];
    __shared__ f32x4 plane[2 * S4 + 1];
    const int tl = threadIdx.x, c = blockIdx.x, C = g.C, H = g.H, W4 = g.W4;
    constexpr int64_t S = 4 * S4;
    unsigned off[KP]; int row[KP], pos[KP];          // byte offset in a plane, row, position in the LDS image of this thread's float4 k
#pragma unroll
    for (int k = 0; k < KP; ++k) { const int j = tl + NT * k; off[k] = 16u * (unsigned)j; row[k] = j / W4; pos[k] = j + row[k] + 1; }
    mid_guards<NT>(plane, H, W4);                    // (visible after the barriers of the first block_sum)
    f32x4 v[MID_BMAX][KP];
#pragma unroll
    for (int b = 0; b < MID_BMAX; ++b) {
        const ws_gptr xb = ws_uniform_base(g.E + ((int64_t)(b < B ? b : 0) * C + c) * S);
#pragma unroll
        for (int k = 0; k < KP; ++k) v[b][k] = ws_load<f32x4>(xb, off[k]);
    }
    __builtin_amdgcn_sched_barrier(0);
    float w[K * K];
#pragma unroll
    for (int i = 0; i < K * K; ++i) w[i] = g.Wdw[(int64_t)c * K * K + i];
    const float n = (float)B * (float)S;
    // BatchNorm0: statistics, running statistics, scale / shift
    float m, q;
    mid_stats<4, KP>(v, B, n, red, m, q);
    float var = q / n;
    if (tl == 0) { g.mean0[c] = m; g.var0[c] = var; mid_running(g.rm0, g.rv0, c, g.mom0, m, q, n); }
    const float sc0 = rsqrtf(var + g.eps0) * g.w0[c], sh0 = g.b0[c] - m * sc0;
    // plane by plane: e' = swish(BatchNorm0(e)) -> LDS -> the depthwise convolution at this thread's own positions -> d (kept in v, written for backward)
#pragma unroll
    for (int b = 0; b < MID_BMAX; ++b) {
        if (b >= B) break;
#pragma unroll
        for (int k = 0; k < KP; ++k) {
            f32x4 o;
            o.x = act_fwd(v[b][k].x * sc0 + sh0, ACT_SWISH); o.y = act_fwd(v[b][k].y * sc0 + sh0, ACT_SWISH);
            o.z = act_fwd(v[b][k].z * sc0 + sh0, ACT_SWISH); o.w = act_fwd(v[b][k].w * sc0 + sh0, ACT_SWISH);
            plane[pos[k]] = o;
        }
        __syncthreads();
        const ws_gptr_w db = ws_uniform_base_w(g.D + ((int64_t)b * C + c) * S);
#pragma unroll
        for (int k = 0; k < KP; ++k) {
            float acc[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int ky = 0; ky < K; ++ky) {
                float e[12];
                mid_window(e, plane, pos[k], row[k], ky - P, H, W4);
#pragma unroll
                for (int j = 0; j < 4; ++j)
#pragma unroll
                    for (int kx = 0; kx < K; ++kx) acc[j] += w[ky * K + kx] * e[4 + j + kx - P];
#pragma unroll
                for (int j = 0; j < 4; ++j) SEGX_PIN(acc[j]);    // as dwconv_rows4_kernel: the chain stays a chain of scalar FMAs next to its LDS reads
            }
            v[b][k] = f32x4{acc[0], acc[1], acc[2], acc[3]};
            ws_store<f32x4>(db, off[k], v[b][k]);
        }
        __syncthreads();                                         // the next plane overwrites the LDS image
        __builtin_amdgcn_sched_barrier(0);                       // one plane at a time (registers)
    }
    // BatchNorm1 on the d still in registers
    mid_stats<4, KP>(v, B, n, red, m, q);
    var = q / n;
    if (tl == 0) { g.mean1[c] = m; g.var1[c] = var; mid_running(g.rm1, g.rv1, c, g.mom1, m, q, n); }
    const float sc1 = rsqrtf(var + g.eps1) * g.w1[c], sh1 = g.b1[c] - m * sc1;
#pragma unroll
    for (int b = 0; b < MID_BMAX; ++b) {
        if (b >= B) break;
        const ws_gptr_w yb = ws_uniform_base_w(g.Y + ((int64_t)b * C + c) * S);
        float acc = 0.f;
#pragma unroll
        for (int k = 0; k < KP; ++k) {
            f32x4 o;
            o.x = act_fwd(v[b][k].x * sc1 + sh1, ACT_SWISH); o.y = act_fwd(v[b][k].y * sc1 + sh1, ACT_SWISH);
            o.z = act_fwd(v[b][k].z * sc1 + sh1, ACT_SWISH); o.w = act_fwd(v[b][k].w * sc1 + sh1, ACT_SWISH);
            ws_store<f32x4>(yb, off[k], o);
            acc += (o.x + o.y) + (o.z + o.w);
        }
        acc = block_sum<4>(acc, red);
        if (tl == 0) g.psum[(int64_t)b * C + c] = acc;           // ONE pooling chunk per plane, the layout segx_se_fwd2 adds up (nch = 1)
        __builtin_amdgcn_sched_barrier(0);
    }
}

// The backward channel sums run over B * H * W <= 24 576 products each; added in fp32 their rounding (~ eps * sqrt(sum of squares) per level of the tree) is as large as
// the error the terms themselves carry.  They are few, so they are added in double: per thread, across the wave, across the workgroup
// (common.h: wave_sum_d, block_sum_d).
struct MidBwdArgs {
    const float* dY; const float* dpool; const float* D; const float* E;
    const float* mean0; const float* var0; const float* mean1; const float* var1;
    const float* w0; const float* b0; const float* w1; const float* b1; const float* Wdw;
    float* dE; float* dw0; float* db0; float* dw1; float* db1; float* dWdw;
    float inv_S, eps0, eps1; int C, H, W4;
};
// grid = C workgroups of NT threads; a plane is NT * KP float4.  dY is the gradient w.r.t. d'; the squeeze-excite pooling adds dpool[b][c] * inv_S to it.
// HL: the xhat planes live in LDS instead of registers (each thread reads and writes only its own slots: no barrier).  The 4096-float planes take it with 1024
// threads: one float4 per thread and plane, 24 instead of 48 resident registers, so the workgroup -- the only one its CU holds either way -- runs four waves per SIMD.
template <int NT, int KP, int K, bool HL>
__global__ __launch_bounds__(NT) void mbconv_mid_bwd_kernel(MidBwdArgs g, int B) {
    constexpr int NW = NT / 64, P = K / 2, S4 = NT * KP, KK = K * K;
    __shared__ double red[NW];
    __shared__ double wred[NW][KK];
    __shared__ f32x4 plane[2 * S4 + 1];
    __shared__ f32x4 hl[HL ? MID_BMAX * S4 : 1];
    const int tl = threadIdx.x, c = blockIdx.x, C = g.C, H = g.H, W4 = g.W4;
    constexpr int64_t S = 4 * S4;
    unsigned off[KP]; int row[KP], pos[KP];          // byte offset in a plane, row, position in the LDS image of this thread's float4 k
#pragma unroll
    for (int k = 0; k < KP; ++k) { const int j = tl + NT * k; off[k] = 16u * (unsigned)j; row[k] = j / W4; pos[k] = j + row[k] + 1; }
    mid_guards<NT>(plane, H, W4);                    // (visible after the barriers of the first block_sum)
    f32x4 h[MID_BMAX][KP], d[MID_BMAX][KP];          // (d, dy) as loaded -> (xhat1, du1) -> per plane (xhat0, du0); HL: h is dead once xhat1 sits in LDS
    auto hget = [&](int b, int k) -> f32x4 { if constexpr (HL) return hl[(b * KP + k) * NT + tl]; else return h[b][k]; };
    auto hput = [&](int b, int k, f32x4 x) { if constexpr (HL) hl[(b * KP + k) * NT + tl] = x; else h[b][k] = x; };
#pragma unroll
    for (int b = 0; b < MID_BMAX; ++b) {
        const int64_t po = ((int64_t)(b < B ? b : 0) * C + c) * S;
        const ws_gptr xb = ws_uniform_base(g.D + po), gb = ws_uniform_base(g.dY + po);
#pragma unroll
        for (int k = 0; k < KP; ++k) { h[b][k] = ws_load<f32x4>(xb, off[k]); d[b][k] = ws_load<f32x4>(gb, off[k]); }
    }
    f32x4 ev[KP];                                    // e of the plane worked on; the next plane's is requested as soon as this one's has been used
    {
        const ws_gptr eb = ws_uniform_base(g.E + (int64_t)c * S);
#pragma unroll
        for (int k = 0; k < KP; ++k) ev[k] = ws_load<f32x4>(eb, off[k]);
    }
    __builtin_amdgcn_sched_barrier(0);
    float w[KK], dwa[KK];
#pragma unroll
    for (int i = 0; i < KK; ++i) { w[i] = g.Wdw[(int64_t)c * KK + i]; dwa[i] = 0.f; }
    const double inv_n = 1.0 / ((double)B * (double)S);
    // 1. BatchNorm1 + swish backward: xhat1, du1 in place, the two channel sums (bn_res_bwd_tail of backbone.hip without gate and drop_connect)
    const float rstd1 = rsqrtf(g.var1[c] + g.eps1), m1 = g.mean1[c], w1c = g.w1[c], b1c = g.b1[c];
    double a = 0.0, q = 0.0;
#pragma unroll
    for (int b = 0; b < MID_BMAX; ++b) {
        const bool bok = b < B;
        const float dp = g.dpool[(bok ? b : 0) * C + c] * g.inv_S;     // (no branch here: a second basic block lets the scheduler pool every plane's arithmetic behind the barriers)
#pragma unroll
        for (int k = 0; k < KP; ++k) {
            const f32x4 xv = h[b][k], gv = d[b][k];
            f32x4 hh, dd;
            hh.x = (xv.x - m1) * rstd1; hh.y = (xv.y - m1) * rstd1; hh.z = (xv.z - m1) * rstd1; hh.w = (xv.w - m1) * rstd1;
            dd.x = (gv.x + dp) * act_grad(hh.x * w1c + b1c, ACT_SWISH); dd.y = (gv.y + dp) * act_grad(hh.y * w1c + b1c, ACT_SWISH);
            dd.z = (gv.z + dp) * act_grad(hh.z * w1c + b1c, ACT_SWISH); dd.w = (gv.w + dp) * act_grad(hh.w * w1c + b1c, ACT_SWISH);
            if (!bok) { dd = f32x4{0.f, 0.f, 0.f, 0.f}; hh = dd; }
            hput(b, k, hh); d[b][k] = dd;
            a += (double)((dd.x + dd.y) + (dd.z + dd.w)); q += (double)((dd.x * hh.x + dd.y * hh.y) + (dd.z * hh.z + dd.w * hh.w));
        }
        __builtin_amdgcn_sched_barrier(0);
    }
    a = block_sum_d<NW>(a, red); q = block_sum_d<NW>(q, red);
    if (tl == 0) { g.db1[c] = (float)a; g.dw1[c] = (float)q; }
    // The gradient w.r.t. d feeds the convolution and BatchNorm0's sums: every rounding in it comes back multiplied by the filter and added up over the channel.
    // For the 4096-float planes (HL) it is formed in double from the fp32 du1, xhat1 and the double means and rounded ONCE (four fp32 roundings per element otherwise:
    // they were the largest single share of the error of dw0 / db0 there).  For the 1024-float planes the three-op route runs bn_act_bwd_res_kernel with this very lane
    // mapping: the fp32 expression of that kernel is kept, so the gradient -- and with it the rounding every later sum inherits -- stays that route's to the last bits.
    const double k1 = a * inv_n, k2 = q * inv_n, sc1 = (double)(w1c * rstd1);
    const float k1f = (float)k1, k2f = (float)k2, sc1f = w1c * rstd1;
    const float rstd0 = rsqrtf(g.var0[c] + g.eps0), m0 = g.mean0[c], sc0 = rstd0 * g.w0[c], sh0 = g.b0[c] - m0 * sc0;       // sc0, sh0: the forward's bits
    double a0 = 0.0, q0 = 0.0;
    // 2.-4. plane by plane: dd (gradient w.r.t. d) -> LDS; around each of its float4s a thread reads the K x K window of dd ONCE for both the data gradient
    //   de'[p] = sum_t w[t] dd[p - t]   and its share of the filter gradient   dW[t] += e'[p] dd[p - t]   (t = tap offset; e' recomputed from e);
    //   then BatchNorm0 + swish backward's du0, xhat0 replace the plane's (du1, xhat1) in registers
#pragma unroll
    for (int b = 0; b < MID_BMAX; ++b) {
        if (b >= B) break;
#pragma unroll
        for (int k = 0; k < KP; ++k) {
            const f32x4 hh = hget(b, k);
            f32x4 o;
            if constexpr (HL) {
                o.x = (float)(sc1 * ((double)d[b][k].x - k1 - (double)hh.x * k2)); o.y = (float)(sc1 * ((double)d[b][k].y - k1 - (double)hh.y * k2));
                o.z = (float)(sc1 * ((double)d[b][k].z - k1 - (double)hh.z * k2)); o.w = (float)(sc1 * ((double)d[b][k].w - k1 - (double)hh.w * k2));
            } else {
                o.x = sc1f * (d[b][k].x - k1f - hh.x * k2f); o.y = sc1f * (d[b][k].y - k1f - hh.y * k2f);
                o.z = sc1f * (d[b][k].z - k1f - hh.z * k2f); o.w = sc1f * (d[b][k].w - k1f - hh.w * k2f);
            }
            plane[pos[k]] = o;
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < KP; ++k) {
            const f32x4 xv = ev[k];
            const float u[4] = {xv.x * sc0 + sh0, xv.y * sc0 + sh0, xv.z * sc0 + sh0, xv.w * sc0 + sh0};
            float ep[4], de[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int i = 0; i < 4; ++i) ep[i] = act_fwd(u[i], ACT_SWISH);
#pragma unroll
            for (int ry = -P; ry <= P; ++ry) {
                float e[12];
                mid_window(e, plane, pos[k], row[k], ry, H, W4);
#pragma unroll
                for (int rx = -P; rx <= P; ++rx) {
                    const int t = (P - ry) * K + (P - rx);     // dd[p + (ry, rx)] reached p through tap (P - ry, P - rx)
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        de[i] = __builtin_fmaf(w[t], e[4 + i + rx], de[i]); dwa[t] = __builtin_fmaf(ep[i], e[4 + i + rx], dwa[t]);
                        SEGX_PIN(de[i]); SEGX_PIN(dwa[t]);     // scalar FMAs: paired into v_pk_fma_f32 the chains needed 450 register moves and spilled 500 bytes per lane
                    }
                }
                __builtin_amdgcn_sched_barrier(0);             // one window row at a time: hoisting all K rows' LDS reads spills the resident planes
            }
            f32x4 hh, dd;
            hh.x = (xv.x - m0) * rstd0; hh.y = (xv.y - m0) * rstd0; hh.z = (xv.z - m0) * rstd0; hh.w = (xv.w - m0) * rstd0;
            dd.x = de[0] * act_grad(u[0], ACT_SWISH); dd.y = de[1] * act_grad(u[1], ACT_SWISH);
            dd.z = de[2] * act_grad(u[2], ACT_SWISH); dd.w = de[3] * act_grad(u[3], ACT_SWISH);
            hput(b, k, hh); d[b][k] = dd;
            a0 += (double)((dd.x + dd.y) + (dd.z + dd.w)); q0 += (double)((dd.x * hh.x + dd.y * hh.y) + (dd.z * hh.z + dd.w * hh.w));
        }
        if (b + 1 < MID_BMAX) {
            const ws_gptr eb = ws_uniform_base(g.E + ((int64_t)(b + 1 < B ? b + 1 : b) * C + c) * S);
#pragma unroll
            for (int k = 0; k < KP; ++k) ev[k] = ws_load<f32x4>(eb, off[k]);
        }
        __syncthreads();                                         // the next plane overwrites the LDS image
        __builtin_amdgcn_sched_barrier(0);
    }
    a0 = block_sum_d<NW>(a0, red); q0 = block_sum_d<NW>(q0, red);
    if (tl == 0) { g.db0[c] = (float)a0; g.dw0[c] = (float)q0; }
    const float j1 = (float)(a0 * inv_n), j2 = (float)(q0 * inv_n);
#pragma unroll
    for (int b = 0; b < MID_BMAX; ++b) {
        if (b >= B) break;
        const ws_gptr_w ob = ws_uniform_base_w(g.dE + ((int64_t)b * C + c) * S);
#pragma unroll
        for (int k = 0; k < KP; ++k) {
            const f32x4 hh = hget(b, k);
            f32x4 o;
            o.x = sc0 * (d[b][k].x - j1 - hh.x * j2); o.y = sc0 * (d[b][k].y - j1 - hh.y * j2);
            o.z = sc0 * (d[b][k].z - j1 - hh.z * j2); o.w = sc0 * (d[b][k].w - j1 - hh.w * j2);
            ws_store<f32x4>(ob, off[k], o);
        }
        __builtin_amdgcn_sched_barrier(0);
    }
    // the filter gradient is complete in this workgroup: waves in order, no partials outside
#pragma unroll
    for (int i = 0; i < KK; ++i) { const double s = wave_sum_d((double)dwa[i]); if ((tl & 63) == 0) wred[tl >> 6][i] = s; }
    __syncthreads();
    if (tl < KK) {
        double s = 0.0;
#pragma unroll
        for (int i = 0; i < NW; ++i) s += wred[i][tl];
        g.dWdw[(int64_t)c * KK + tl] = (float)s;
    }
}

static inline bool mid_serves(int B, int C, int H, int W, int k) {
    return B >= 1 && B <= MID_BMAX && C >= 1 && H >= 1 && W >= 4 && W % 4 == 0 && (k == 3 || k == 5) && ((int64_t)H * W == 1024 || (int64_t)H * W == 4096);
}
static inline bool mid_aligned(std::initializer_list<const void*> ps) {
    for (const void* p : ps) if (reinterpret_cast<uintptr_t>(p) & 15) return false;
    return true;
}

}  // namespace segx

using namespace segx;
#define SEGX_STREAM hipStream_t stream = (hipStream_t)stream_

extern "C" int segx_mbconv_mid_ok(int B, int C, int H, int W, int k) { return mid_serves(B, C, H, W, k) ? 1 : 0; }

extern "C" int segx_mbconv_mid_fwd(const float* E, const float* w0, const float* b0, float* run_mean0, float* run_var0, const float* Wdw, const float* w1, const float* b1,
                                   float* run_mean1, float* run_var1, float* D, float* Y, float* psum, float* mean0, float* var0, float* mean1, float* var1,
                                   float momentum0, float eps0, float momentum1, float eps1, int B, int C, int H, int W, int k, void* stream_) {
    SEGX_STREAM; SEGX_REQUIRE(E && w0 && b0 && Wdw && w1 && b1 && D && Y && psum && mean0 && var0 && mean1 && var1 && (!run_mean0 == !run_var0) && (!run_mean1 == !run_var1),
                              "segx_mbconv_mid_fwd: bad args");
    SEGX_REQUIRE(mid_serves(B, C, H, W, k), "segx_mbconv_mid_fwd: shape not served (segx_mbconv_mid_ok == 0)");
    SEGX_REQUIRE(mid_aligned({E, D, Y}), "segx_mbconv_mid_fwd: tensors must be 16-byte aligned");
    const MidFwdArgs g{E, w0, b0, run_mean0, run_var0, Wdw, w1, b1, run_mean1, run_var1, D, Y, psum, mean0, var0, mean1, var1, momentum0, eps0, momentum1, eps1, C, H, W / 4};
#define SEGX_MID_F(KP, K) hipLaunchKernelGGL((mbconv_mid_fwd_kernel<KP, K>), dim3((unsigned)C), dim3(256), 0, stream, g, B)
    if (H * W == 4096) { if (k == 3) SEGX_MID_F(4, 3); else SEGX_MID_F(4, 5); }
    else { if (k == 3) SEGX_MID_F(1, 3); else SEGX_MID_F(1, 5); }
#undef SEGX_MID_F
    return check_launch("segx_mbconv_mid_fwd");
}

extern "C" int segx_mbconv_mid_bwd(const float* dY, const float* dpool, const float* D, const float* E, const float* mean0, const float* var0, const float* mean1,
                                   const float* var1, const float* w0, const float* b0, const float* w1, const float* b1, const float* Wdw,
                                   float* dE, float* dw0, float* db0, float* dw1, float* db1, float* dWdw, float inv_S, float eps0, float eps1,
                                   int B, int C, int H, int W, int k, void* stream_) {
    SEGX_STREAM; SEGX_REQUIRE(dY && dpool && D && E && mean0 && var0 && mean1 && var1 && w0 && b0 && w1 && b1 && Wdw && dE && dw0 && db0 && dw1 && db1 && dWdw, "segx_mbconv_mid_bwd: bad args");
    SEGX_REQUIRE(mid_serves(B, C, H, W, k), "segx_mbconv_mid_bwd: shape not served (segx_mbconv_mid_ok == 0)");
    SEGX_REQUIRE(mid_aligned({dY, D, E, dE}), "segx_mbconv_mid_bwd: tensors must be 16-byte aligned");
    const MidBwdArgs g{dY, dpool, D, E, mean0, var0, mean1, var1, w0, b0, w1, b1, Wdw, dE, dw0, db0, dw1, db1, dWdw, inv_S, eps0, eps1, C, H, W / 4};
#define SEGX_MID_B(NT, KP, K, HL) hipLaunchKernelGGL((mbconv_mid_bwd_kernel<NT, KP, K, HL>), dim3((unsigned)C), dim3(NT), 0, stream, g, B)
    if (H * W == 4096) { if (k == 3) SEGX_MID_B(1024, 1, 3, true); else SEGX_MID_B(512, 2, 5, true); }     // k = 5 at 1024 threads spills 76 bytes under the 128-register cap
    else { if (k == 3) SEGX_MID_B(256, 1, 3, false); else SEGX_MID_B(256, 1, 5, false); }
#undef SEGX_MID_B
    return check_launch("segx_mbconv_mid_bwd");
}
