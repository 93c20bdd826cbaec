// gemm.hip -- batched strided fp32 GEMM on the gfx950 f32 matrix core (v_mfma_f32_32x32x2_f32).
//
// Why f32 MFMA: the parity bar is fp32-faithful logits (bf16 MFMA inputs flip hardened
// labels), and gfx950 has no TF32.  v_mfma_f32_32x32x2_f32 is bit-for-bit a k-ordered fmaf chain and
// peaks at 157.3 TFLOP/s -- the roofline this kernel is measured against.
//
// Tiling: workgroup = 256 threads = 4 waves (2x2); block tile 128x128, k-tile 32; each wave owns a
// 64x64 sub-tile = 2x2 MFMA tiles of 32x32 (4 x f32x16 accumulators = 64 VGPRs).  Both operand tiles are
// staged through LDS k-major ([k][m], row stride 132 floats) so that an MFMA operand fetch is one
// conflict-free ds_read_b32 per lane (lane l needs A[m0 + (l&31)][k0 + (l>>5)]).  The next k-tile's
// global loads (4 x float4 per operand per thread) are issued before the 64 MFMAs of the current tile
// and written to LDS after them, so HBM/L2 latency hides under ~4k cycles of matrix work per wave.
// One MFMA occupies its SIMD for 64 cycles, so 4 LDS reads per 4 MFMAs keep LDS traffic at a few %
// of the matrix-pipe time; >= 2 workgroups per CU cover each other's barriers.
//
// Operands are addressed through (batch0, batch1, row, k) element strides, one of (row, k) being 1:
//   K-contiguous operand -> float4 along k, transposing scalar LDS stores;
//   row-contiguous operand -> float4 along rows, float4 LDS stores.
// All four combinations (NT: linear fwd / QK^T, NN: P.V, dX = dY.W; TN: dW = dY^T.X; TT) are
// instantiated, so no operand is ever materialised transposed in HBM.
#include "gemm_x6ws.h"
#include "gemm_skinny.h"
#include "gemm_tuned.h"

namespace segx {

template <class Cfg, bool AKC, bool BKC, bool VEC, int EPI>
__global__ __launch_bounds__(256, 2) void gemm_f32_kernel(GemmArgs g) {
    __shared__ __attribute__((aligned(16))) TileLdsT<Cfg> lds;
    const TileCoord t = tile_coord<Cfg>(g);
    const DenseLoader<AKC, VEC, Cfg::BM> la{g.A + t.z0 * g.a_b0 + t.z1 * g.a_b1, g.a_m, g.a_k, t.m0, g.M};
    const DenseLoader<BKC, VEC, Cfg::BN> lb{g.B + t.z0 * g.b_b0 + t.z1 * g.b_b1, g.b_n, g.b_k, t.n0, g.N};
    f32x16 acc[Cfg::MI][Cfg::NJ];
    gemm_mainloop<Cfg>(acc, la, lb, t.kbeg, t.kend, lds);
    gemm_epilogue<EPI, Cfg>(acc, g, t);
}

// The same GEMM on the bf16x6 engine (gemm_x6.h): fp32 operands split into three bf16 planes on their way into LDS, six bf16 MFMAs per
// block and 16 k.  WPE = resident waves per SIMD the register allocation must allow (LDS: 48 / 36 / 24 KB per workgroup).
// TERMS = 3: the three-term product (two planes per operand: 32 / 24 / 16 KB per workgroup), segx_tune knob 20.
template <class Cfg, bool AKC, bool BKC, int EPI, int WPE, int VAR = 0, int TERMS = 6>
__global__ __launch_bounds__(256) SEGX_MIN_WAVES_PER_SIMD(WPE) void gemm_x6_kernel(GemmArgs g) {
    __shared__ __attribute__((aligned(16))) unsigned char lds[X6Lds<Cfg, TERMS>::BYTES];
    const TileCoord t = tile_coord<Cfg>(g);
    const DenseLoader6<AKC, Cfg::BM> la{g.A + t.z0 * g.a_b0 + t.z1 * g.a_b1, g.a_m, g.a_k, t.m0, g.M};
    const DenseLoader6<BKC, Cfg::BN> lb{g.B + t.z0 * g.b_b0 + t.z1 * g.b_b1, g.b_n, g.b_k, t.n0, g.N};
    f32x16 acc[Cfg::MI][Cfg::NJ];
    gemm_mainloop_x6<Cfg, DenseLoader6<AKC, Cfg::BM>, DenseLoader6<BKC, Cfg::BN>, VAR, TERMS>(acc, la, lb, t.kbeg, t.kend, lds);
    gemm_epilogue<EPI, Cfg>(acc, g, t);
}

// The 4-wave kernel with the LEAN operand loaders of gemm_x6ws.h (one uniform base per k-tile + a 32-bit offset per piece computed once per tile:
// no per-k-tile address arithmetic on the vector pipe -- ~80 of the ~280 vector instructions a thread issued per k-tile).  Whole 32-k tiles and
// 32-bit operand offsets only (gemm_ws_ok): the host keeps gemm_x6_kernel for everything else.
template <class Cfg, bool AKC, bool BKC, int EPI, int WPE, int TERMS = 6>
__global__ __launch_bounds__(256) SEGX_MIN_WAVES_PER_SIMD(WPE) void gemm_x6_lean_kernel(GemmArgs g) {
    __shared__ __attribute__((aligned(16))) unsigned char lds[X6Lds<Cfg, TERMS>::BYTES];
    const TileCoord t = tile_coord<Cfg>(g);
    WsDense6<AKC, Cfg::BM> la; WsDense6<BKC, Cfg::BN> lb;
    la.begin(g.A + t.z0 * g.a_b0 + t.z1 * g.a_b1, g.a_m, g.a_k, t.m0, g.M, threadIdx.x);
    lb.begin(g.B + t.z0 * g.b_b0 + t.z1 * g.b_b1, g.b_n, g.b_k, t.n0, g.N, threadIdx.x);
    f32x16 acc[Cfg::MI][Cfg::NJ];
    gemm_mainloop_x6<Cfg, WsDense6<AKC, Cfg::BM>, WsDense6<BKC, Cfg::BN>, 0, TERMS>(acc, la, lb, t.kbeg, t.kend, lds);
    gemm_epilogue<EPI, Cfg>(acc, g, t);
}

// The wave-specialised persistent form (gemm_x6ws.h): 512 threads, one workgroup per CU (144 / 96 KB of LDS), grid = min(items, 256).
template <class Cfg, bool AKC, bool BKC, int EPI, int PRIO = 0, int TERMS = 6>
__global__ __launch_bounds__(512) void gemm_x6ws_kernel(GemmArgs g) {
    __shared__ __attribute__((aligned(16))) unsigned char lds[X6WsLds<Cfg, TERMS>::BYTES];
    x6ws_body<Cfg, DenseMk6<Cfg, AKC, BKC>, EPI, PRIO, TERMS>(g, DenseMk6<Cfg, AKC, BKC>{}, lds);
}

// ... with the B operand split ahead of time (segx_x6_presplit; WsPre6): plain epilogue, whole 32-k stages, 256- or 128-row B tiles
template <class Cfg, bool AKC>
__global__ __launch_bounds__(512) void gemm_x6ws_pre_kernel(GemmArgs g) {
    __shared__ __attribute__((aligned(16))) unsigned char lds[X6WsLds<Cfg>::BYTES];
    x6ws_body<Cfg, PreMk6<Cfg, AKC>, SEGX_EPI_NONE, 0>(g, PreMk6<Cfg, AKC>{}, lds);
}

// fp32 operand [nb][rows][K] (any of the two unit-stride layouts) -> three bf16 planes [nb][plane][rows][K], k contiguous: x = hi + mid + lo with the
// rounding of split3_pair.  A thread owns 8 consecutive k of one row.  Threads run along k for k-contiguous input (coalesced loads and stores), along the
// rows for row-contiguous input (coalesced loads, 16-byte stores one row apart: weights only, a few MB).
__global__ __launch_bounds__(256) void x6_presplit_kernel(const float* __restrict__ W, unsigned short* __restrict__ P, int rows, int K, int64_t s_row, int64_t s_k,
                                                          int nb1, int64_t s_b0, int64_t s_b1, int64_t per_batch) {
    const int kch = K >> 3;
    const int z = blockIdx.y, z0 = z / nb1, z1 = z - z0 * nb1;
    const float* __restrict__ w = W + z0 * s_b0 + z1 * s_b1;
    unsigned short* __restrict__ o = P + (int64_t)z * 3 * per_batch;
    for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < per_batch / 8; idx += (int64_t)gridDim.x * blockDim.x) {
        int row, kc;
        if (s_k == 1) { row = (int)(idx / kch); kc = (int)(idx - (int64_t)row * kch); }
        else { kc = (int)(idx / rows); row = (int)(idx - (int64_t)kc * rows); }
        float v[8];
        const float* src = w + (int64_t)row * s_row + (int64_t)(kc * 8) * s_k;
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = src[(int64_t)j * s_k];
        const Split2 a = split3_pair(v[0], v[1]), b = split3_pair(v[2], v[3]), c = split3_pair(v[4], v[5]), d = split3_pair(v[6], v[7]);
        const int64_t e = (int64_t)row * K + kc * 8;
        *reinterpret_cast<uint4*>(o + e) = make_uint4(a.h, b.h, c.h, d.h);
        *reinterpret_cast<uint4*>(o + per_batch + e) = make_uint4(a.m, b.m, c.m, d.m);
        *reinterpret_cast<uint4*>(o + 2 * per_batch + e) = make_uint4(a.l, b.l, c.l, d.l);
    }
}

// The same reduction for MANY slabs over a SMALL output (batch_reduce of the skinny weight gradients: 6 x 63 slabs of 24 x 144 floats): the slab
// loop is dealt out over PARTS threads per output element (slab s -> part s % PARTS, each part in slab order) and the PARTS partial sums are
// added in part order through LDS -- a fixed summation tree, so still deterministic; 256 / PARTS outputs per workgroup.
template <int PARTS>
__global__ __launch_bounds__(256) void slab_sum_parts_kernel(const float* __restrict__ ws, float* __restrict__ C, const float* __restrict__ bias,
                                                             int M, int N, int nslabs, int64_t total, int64_t c_m, float alpha, int bias_mode) {
    __shared__ float part[256];
    constexpr int EPB = 256 / PARTS;
    const int e = threadIdx.x % EPB, pt = threadIdx.x / EPB;
    const int64_t idx = (int64_t)blockIdx.x * EPB + e;
    float s = 0.f;
    if (idx < total) for (int k = pt; k < nslabs; k += PARTS) s += ws[(int64_t)k * total + idx];
    part[threadIdx.x] = s;
    __syncthreads();
    if (pt == 0 && idx < total) {
        float t = 0.f;
#pragma unroll
        for (int q = 0; q < PARTS; ++q) t += part[q * EPB + e];
        t *= alpha;
        const int col = (int)(idx % N), row = (int)(idx / N);
        if (bias_mode == SEGX_BIAS_N) t += bias[col]; else if (bias_mode == SEGX_BIAS_M) t += bias[row];
        C[(int64_t)row * c_m + col] = t;
    }
}

static bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// Tile / split-K planning.  Skinny operands are a rule (measured, tools/gemm_bench.py tiles, r01-j): an operand with <= 48 rows
// is streamed with the 32-row tile on that side -- the 128-row tile spends 3/4 of its LDS traffic and MFMA issue slots on
// clamped duplicate rows (192x32x65536 weight gradient: 0.34 -> 0.14 ms).  Everything else is priced with a small model:
//   time = rounds of workgroups over the resident slots x (k-tiles x step time + prologue/epilogue) + split-K slab reduction
// Whole-GEMM quantisation matters (784 workgroups on 768 slots take two rounds, not 1.02), and so do padded edge tiles, which
// the workgroup count already contains.  Step times are the measured ~112 TFLOP/s of the engine expressed per k-tile.
// splitk_fixed > 0: the caller has already chosen the split factor; 0: choose it too.  vec = false: only the default tile is built.
// bf16x6 engine: float4-legal operands, neither side skinny (those GEMMs are HBM-bound and stream through the 32-row fp32 tiles)
// the engine of ONE call: segx_gemm_desc.engine (SEGX_ENGINE_SEL_F32 / _BF16X6) or, at SEGX_ENGINE_SEL_DEFAULT, the process default (segx_tune knob 4)
static int call_engine(const segx_gemm_desc* d) {
    return d->engine == SEGX_ENGINE_SEL_F32 ? SEGX_ENGINE_F32 : d->engine == SEGX_ENGINE_SEL_BF16X6 ? SEGX_ENGINE_BF16X6 : kget(knobs().engine);
}
static bool x6_eligible(int engine, int M, int N, bool vec) { return engine == SEGX_ENGINE_BF16X6 && vec && M > 48 && N > 48; }
// The pricing step of both planners: one candidate tile at the split factor the caller fixed (1 where the call may not split), or at the best one.
// ws_grid > 0: the candidate is a wave-specialised tile, priced as a persistent launch of that many workgroups.  Returns the split factor, *t its time.
static int price(const TileInfo& c, int M, int N, int K, int nbatch, bool may_split, int splitk_fixed, int ws_grid, double* t) {
    const TileInfo6 c6{c.id, c.bm, c.bn, c.wg_per_cu, c.ktile_us, c.fixed_us};
    if (splitk_fixed > 0 || !may_split) {
        const int sk = splitk_fixed > 0 ? splitk_fixed : 1;
        *t = ws_grid > 0 ? model_us_ws(c6, M, N, K, nbatch, sk, ws_grid) : model_us(c, M, N, K, nbatch, sk);
        return sk;
    }
    return ws_grid > 0 ? best_splitk_ws(c6, M, N, K, nbatch, ws_grid, t) : best_splitk(c, M, N, K, nbatch, t);
}
// ws_ok: the wave-specialised persistent kernels may run this GEMM (whole 32-k stages, 32-bit operand offsets; no fused GELU: its epilogue
// runs on four of the eight waves there and measured 63 against 91 TFLOP/s)
// nrc = number of row-contiguous operands (0..2): their loaders cost the 4-wave kernels 9 % / 34 % per k-tile (r03_f: 201 / 185 / 150 TFLOP/s for
// NT / NN / TN at 24576 x 1792 x 1792), the wave-specialised ones 1 % / 5 % (220 / 218 / 198 incl. the slab reduction)
static void plan6(int M, int N, int K, int nbatch, bool gelu, bool may_split, int splitk_fixed, bool ws_ok, int nrc, int* tile, int* splitk) {   // (the fused swish: ws_ok = false)
    double best_t = -1.0;
    const float f4 = nrc == 0 ? 1.0f : nrc == 1 ? 1.09f : 1.34f, fws = nrc == 0 ? 1.0f : nrc == 1 ? 1.01f : 1.05f;
    for (const TileInfo6& c6 : kTiles6) {
        if (gelu && c6.id != SEGX_TILE_128x128) continue;                  // the fused GELU epilogue is built for the default tile
        double t;
        const int sk = price(TileInfo{c6.id, c6.bm, c6.bn, c6.wg_per_cu, c6.ktile_us * f4, c6.fixed_us}, M, N, K, nbatch, may_split, splitk_fixed, 0, &t);
        if (best_t < 0.0 || t < best_t * 0.97) { best_t = t; *tile = c6.id; *splitk = sk; }
    }
    if (!ws_ok || gelu) return;
    for (const TileInfo6& w6 : kTilesWs) {
        double t;
        const int sk = price(TileInfo{w6.id, w6.bm, w6.bn, w6.wg_per_cu, w6.ktile_us * fws, w6.fixed_us}, M, N, K, nbatch, may_split, splitk_fixed, kget(knobs().ws_grid), &t);
        if (t < best_t * 0.97) { best_t = t; *tile = w6.id; *splitk = sk; }
    }
}
// whole 32-k stages and 32-bit operand offsets: what the lean loaders (4-wave lean kernels, wave-specialised kernels) need
static bool gemm_lean_ok(const segx_gemm_desc* d) {
    const bool akc = (d->a_k == 1), bkc = (d->b_k == 1);
    const int64_t a_span = akc ? (int64_t)d->M * d->a_m : (int64_t)d->K * d->a_k, b_span = bkc ? (int64_t)d->N * d->b_n : (int64_t)d->K * d->b_k;
    return d->K % BKT == 0 && a_span < (1LL << 29) && b_span < (1LL << 29);
}
// a residual operand keeps the call on the 4-wave kernels: their epilogue reads it as 16-byte quads next to the 16-byte stores, the wave-specialised
// kernels' 4-byte epilogue would read it scalar (r04_c: the 160 x 4096 x 960 x 6 dX GEMM 0.47 -> 0.76 ms/step with the residual on the 256 x 128 tile)
static bool gemm_ws_ok(const segx_gemm_desc* d) { return !d->resid && gemm_lean_ok(d); }
// skinny_ok = false: the 32-row tiles are not built for this call's epilogue (the fused swish)
static void plan(int M, int N, int K, int nbatch, bool vec, bool may_split, int splitk_fixed, int* tile, int* splitk, bool skinny_ok = true) {
    const TileInfo* cand[3]; int nc = 0;
    if (!vec) cand[nc++] = &kTiles[0];
    else if (skinny_ok && N <= 48 && M > N) cand[nc++] = &tile_info(SEGX_TILE_128x32);
    else if (skinny_ok && M <= 48) cand[nc++] = &tile_info(SEGX_TILE_32x128);
    else { cand[nc++] = &kTiles[0]; cand[nc++] = &kTiles[1]; cand[nc++] = &kTiles[2]; }
    double best_t = -1.0;
    for (int i = 0; i < nc; ++i) {
        double t;
        const int sk = price(*cand[i], M, N, K, nbatch, may_split, splitk_fixed, 0, &t);
        if (best_t < 0.0 || t < best_t * 0.97) { best_t = t; *tile = cand[i]->id; *splitk = sk; }   // larger tiles win ties
    }
}
static bool gemm_vec_ok(const float* A, const float* B, const segx_gemm_desc* d) {
    const bool akc = (d->a_k == 1), bkc = (d->b_k == 1);
    // float4 loads need 16-B aligned bases, every non-unit stride and the contiguous extents multiples of 4
    const bool vecA = aligned16(A) && (d->a_b0 % 4 == 0) && (d->a_b1 % 4 == 0) && ((akc ? d->a_m : d->a_k) % 4 == 0) &&
                      ((akc ? d->K : d->M) % 4 == 0);
    const bool vecB = aligned16(B) && (d->b_b0 % 4 == 0) && (d->b_b1 % 4 == 0) && ((bkc ? d->b_n : d->b_k) % 4 == 0) &&
                      ((bkc ? d->K : d->N) % 4 == 0);
    return vecA && vecB;
}
// the streaming skinny weight gradient (gemm_skinny.hip): batch-reduced, both operands k-contiguous and float4-legal, plain epilogue, one side <= 32 rows;
// slabs = the largest multiple of the batch size under the persistent grid (the caller's workspace is splitk x nbatch slabs)
static int skinny_nt_splitk(const float* A, const float* B, const segx_gemm_desc* d) {
    if (!kget(knobs().skinny_nt) || !d->batch_reduce || d->epilogue != SEGX_EPI_NONE || d->gmax || d->resid || d->a_k != 1 || d->b_k != 1) return 0;
    if (!gemm_vec_ok(A, B, d)) return 0;
    const int nbatch = d->nb0 * d->nb1;
    const int sk = (int)i64max(1, (int64_t)kget(knobs().ws_grid) * skinny_nt_wgs_per_cu(d->M, d->N) / nbatch);
    if (!skinny_nt_shape_ok(d->M, d->N, d->K, nbatch, sk * nbatch)) return 0;
    if ((int64_t)d->M * d->a_m >= (1LL << 31) || (int64_t)d->N * d->b_n >= (1LL << 31)) return 0;          // 32-bit row offsets inside a member
    return sk;
}

static int gemm_plan_impl(const float* A, const float* B, const segx_gemm_desc* d, int* tile, int* splitk, bool use_table) {
    SEGX_REQUIRE(A && B && d && tile && splitk && d->M > 0 && d->N > 0 && d->K > 0 && d->nb0 > 0 && d->nb1 > 0, "segx_gemm_plan: bad args");
    const bool plain = d->epilogue == SEGX_EPI_NONE, swish = d->epilogue == SEGX_EPI_SWISH || d->epilogue == SEGX_EPI_RELU;      // (the fused ReLU is planned, routed and built like the fused swish)
    int t = SEGX_TILE_128x128, sk = 1;
    const bool vec = gemm_vec_ok(A, B, d);
    if (const int ssk = skinny_nt_splitk(A, B, d)) { *tile = SEGX_TILE_SKINNY_NT; *splitk = ssk; return 0; }
    if (use_table && plain && !d->gmax && x6_eligible(call_engine(d), d->M, d->N, vec)) {
        // measured choices first (gemm_tuned.h); a wave-specialised entry still needs its preconditions (they hold for the shapes it was measured on)
        const int nbt = d->nb0 * d->nb1; const bool akc_ = d->a_k == 1, bkc_ = d->b_k == 1;
        for (const TunedGemm& e : kTunedGemm)
            if (e.M == d->M && e.N == d->N && e.K == d->K && e.nb == nbt && (e.akc != 0) == akc_ && (e.bkc != 0) == bkc_) {
                if (e.tile >= SEGX_TILE_256x128 && !gemm_ws_ok(d)) break;
                *tile = e.tile; *splitk = e.splitk;
                return 0;
            }
    }
    // the fused swish is built for the three four-wave tiles of either engine (no wave-specialised, no 32-row tile) and never splits
    if (x6_eligible(call_engine(d), d->M, d->N, vec) && (plain || d->a_k == 1))
        plan6(d->M, d->N, d->K, d->nb0 * d->nb1, !plain && !swish, plain && !d->gmax, 0, gemm_ws_ok(d) && !swish, (d->a_k != 1) + (d->b_k != 1), &t, &sk);
    else plan(d->M, d->N, d->K, d->nb0 * d->nb1, vec && (plain || swish), plain && !d->gmax, 0, &t, &sk, !swish);
    *tile = t; *splitk = sk;
    return 0;
}

// ---- routing: which kernel runs a validated descriptor ----------------------------------------------------------------------------------
enum GemmFamily {
    GEMM_F32,        // gemm_f32_kernel: v_mfma_f32_32x32x2_f32, every layout, float4-legal or not
    GEMM_X6,         // gemm_x6_kernel: bf16x6, four waves
    GEMM_X6_LEAN,    // gemm_x6_lean_kernel: the same with the lean operand loaders
    GEMM_WS,         // gemm_x6ws_kernel: wave-specialised, persistent
    GEMM_WS_PRE,     // gemm_x6ws_pre_kernel: ... with the B operand split ahead of time
    GEMM_SKINNY      // gemm_skinny.hip: streaming batch-reduced weight gradient
};
struct GemmRoute {
    int family;      // GemmFamily
    int tile;        // SEGX_TILE_* the kernel is built for, after every fallback (never AUTO)
    bool akc, bkc;   // A / B k-contiguous
    bool vec;        // float4-legal operands (false: gemm_f32_kernel's scalar loaders, default tile)
    int epi;         // SEGX_EPI_*
    int sched;       // knob 6 as it applies to THIS kernel: 0 = the product schedule (gemm_x6_kernel at the waves per SIMD of its tile); GEMM_X6 on the plain NT
                     // default tile: 1 / 6 / 7 (and the ablations 2..5 in SEGX_BENCH builds); GEMM_WS: 1 (2..5 on the plain NT form in SEGX_BENCH builds)
    int splitk;      // k slabs (GEMM_SKINNY: x the batch size = its slabs = its grid)
    int ws_grid;     // knob 9: most workgroups of a persistent launch (GEMM_WS, GEMM_WS_PRE)
    bool walk;       // knob 19: the tiles may be walked M fastest (set_tiles)
    int terms;       // knob 20 as it applies to THIS kernel: 3 = the three-term bf16 product (x3_built()), 6 = the six-term one; 0 off the bf16 tile engine
};
static bool ws_tile_id(int tile) { return tile >= SEGX_TILE_256x128 && tile <= SEGX_TILE_WS256x96; }
// The routes that have a three-term kernel: those the eval forward of the 2-D model takes (launch counters around every GEMM of cfg1 / cfg2 / cfg3 at the fixture
// and the product shapes, folded and unfolded), all on the product schedule:
//   wave-specialised, plain, A k-contiguous: 256 x 128, 128 x 128, 128 x 256 and 96 x 256 with B in either layout, 64 x 256 with B row-contiguous, 256 x 96;
//   four-wave, dense loaders (K no multiple of 32): A k-contiguous, B row-contiguous -- a pointwise convolution -- plain and fused swish, the three tiles;
//   four-wave, lean loaders: the same; the plain products with a k-contiguous B, A in either layout (NT: nn.Linear, Q.K^T), on all three tiles -- NT on 64 x 128 is
//   the one route the eval forward of the 3-D model added;
//   the fused GELU (128 x 128, A k-contiguous) with B in either layout.
// Every other route runs six-term whatever knob 20 says, and the counters show it (segx_x3_launches).
static bool x3_built(const GemmRoute& r) {
    if (r.sched != 0) return false;
    const bool plain = r.epi == SEGX_EPI_NONE, conv = r.akc && !r.bkc;
    switch (r.family) {
        case GEMM_WS: return plain && r.akc && (r.tile != SEGX_TILE_WS64x256 || !r.bkc);       // 256 x 96 has a k-contiguous B by its route
        case GEMM_X6: return conv && r.epi != SEGX_EPI_GELU;
        case GEMM_X6_LEAN:
            if (!plain) return r.akc;                        // swish: A k-contiguous, B row-contiguous by the entry point's contract; GELU: A k-contiguous
            return conv || r.bkc;                            // (NT on 64 x 128: the [2352 x 1024 x 256] x 16 attention product of the 3-D forward at cfg4's size)
        default: return false;
    }
}

// Pure: reads the descriptor, the operand addresses (alignment only) and the knobs -- every knob a launch depends on is read here -- and launches nothing.
static int gemm_route(const float* A, const float* B, const segx_gemm_desc* d, GemmRoute* out) {
    GemmRoute r;
    r.akc = d->a_k == 1; r.bkc = d->b_k == 1; r.vec = gemm_vec_ok(A, B, d);
    r.epi = d->epilogue; r.sched = 0; r.splitk = d->splitk > 1 ? d->splitk : 1;
    r.ws_grid = kget(knobs().ws_grid); r.walk = kget(knobs().tile_walk) != 0; r.terms = 0;
    const int want_terms = kget(knobs().x6_terms);
    const int nbatch = d->nb0 * d->nb1;
    const bool gelu = d->epilogue == SEGX_EPI_GELU, swish = d->epilogue == SEGX_EPI_SWISH || d->epilogue == SEGX_EPI_RELU, ws_forced = ws_tile_id(d->tile);
    const int engine = call_engine(d);
    SEGX_REQUIRE(!ws_forced || engine == SEGX_ENGINE_BF16X6, "segx_gemm_f32: tile %d exists on the bf16x6 engine only", d->tile);
    int tile = d->tile;
    if (tile == SEGX_TILE_SKINNY_NT) {
        // the plan's slab count travels as splitk; anything the streaming kernel does not serve quietly takes the planner's tile (like the 96-row tiles)
        const int ssk = skinny_nt_splitk(A, B, d);
        if (ssk > 0 && r.splitk <= ssk) { r.family = GEMM_SKINNY; r.tile = tile; *out = r; return 0; }
        tile = SEGX_TILE_AUTO;
    }
    // the wave-specialised kernels address an operand through 32-bit byte offsets from a per-item base and take whole 32-k stages only
    const bool ws_ok = gemm_ws_ok(d);
    // the bf16x6 engine has the default tile, the two 64-row tiles and the wave-specialised ones; its fused GELU is built for a k-contiguous A
    const bool x6 = x6_eligible(engine, d->M, d->N, r.vec) && (!gelu || r.akc) &&
                    (tile == SEGX_TILE_AUTO || tile == SEGX_TILE_128x128 || tile == SEGX_TILE_64x128 || tile == SEGX_TILE_64x64 || ws_forced);
    if (tile == SEGX_TILE_AUTO) {                            // the caller chose the split factor (or 1): the tile is priced for that one
        int sk_unused = 1;
        if (x6) plan6(d->M, d->N, d->K, nbatch, gelu, false, r.splitk, ws_ok && !swish, (!r.akc) + (!r.bkc), &tile, &sk_unused);
        else plan(d->M, d->N, d->K, nbatch, r.vec && !gelu, false, r.splitk, &tile, &sk_unused, !swish);
    }
    // the fused swish / ReLU (a folded pointwise convolution's forward) is built for the three four-wave tiles of either engine: any other tile a caller names takes the default one
    if (swish && tile != SEGX_TILE_64x128 && tile != SEGX_TILE_64x64) tile = SEGX_TILE_128x128;
    if (ws_forced && !ws_ok) tile = SEGX_TILE_128x128;
    // the 96-row tiles (channel counts 272 / 160 / 192 / 672 / 960 of the backbone: 3 x 96 = 288 rows cover 272 where 3 x 128 compute 384) stage their 96-row
    // side with the k-contiguous loader only (the row-contiguous one deals 64 / 128 / 256 rows over a workgroup); no fused GELU
    if ((tile == SEGX_TILE_WS96x256 && (!r.akc || gelu)) || (tile == SEGX_TILE_WS256x96 && (!r.bkc || gelu))) tile = SEGX_TILE_128x128;
    // no fused GELU on the other two few-channel tiles either (pointwise convolutions have none): the default tile's four-wave form runs it
    if (gelu && (tile == SEGX_TILE_WS128x256 || tile == SEGX_TILE_WS64x256)) tile = SEGX_TILE_128x128;
    const bool ws = x6 && ws_ok && ws_tile_id(tile);
    if (!r.vec || (gelu && !ws) || (ws_forced && !x6)) tile = SEGX_TILE_128x128;       // odd shapes / fused GELU: only the default tile (and the wave-specialised ones) are built
    r.tile = tile;
    if (!x6) {
        SEGX_REQUIRE(!gelu || r.akc, "segx_gemm_f32: the GELU epilogue is built for a k-contiguous A operand (nn.Linear, attention fusion)");
        r.family = GEMM_F32;
    } else if (ws) {
        // persistent launch.  Variant 1 = consumers at raised wave priority (same results); the ablation variants 2..5 (results are NOT the GEMM) exist in
        // -DSEGX_BENCH builds only (tools/build_variant.py), for the plain NT form
        const int v = kget(knobs().x6_variant);
        r.sched = v == 1 ? 1 : 0;
#ifdef SEGX_BENCH
        if (v >= 2 && v <= 5 && !gelu && r.akc && r.bkc) r.sched = v;
#endif
        // pre-split B operand (segx_x6_presplit): the wave-specialised 256 x 128 / 128 x 256 kernels with a copy-only B loader; anything else ignores the planes
        const bool pre = d->b_planes && !gelu && (tile == SEGX_TILE_256x128 || tile == SEGX_TILE_WS128x256);
        r.family = pre ? GEMM_WS_PRE : GEMM_WS;
        if (pre) r.sched = 0;
    } else {
        const int v = kget(knobs().x6_variant);
        if (v > 0 && !gelu && r.akc && r.bkc && tile == SEGX_TILE_128x128) {
            r.family = GEMM_X6; r.sched = v;                 // the schedule variants are built on the plain NT default tile with the dense loaders
        } else {
#ifdef SEGX_NO_LEAN                                          // bench-only A/B build (tools/build_variant.py)
            r.family = GEMM_X6;
#else
            r.family = gemm_lean_ok(d) ? GEMM_X6_LEAN : GEMM_X6;
#endif
        }
    }
    if (r.family != GEMM_F32) r.terms = want_terms == 3 && x3_built(r) ? 3 : 6;
    *out = r;
    return 0;
}

// ---- launch: the route's run-time choices -> template arguments.  Only the forms a route can name are instantiated: the 96-row tiles for one layout pair each,
// the fused GELU with a k-contiguous A only, the schedule variants on the plain NT default tile only. ---------------------------------------------------------
using GemmKernel = void (*)(GemmArgs);
struct GemmLaunch { GemmKernel fn; int bm, bn; };            // bm x bn: the tile the kernel was instantiated for
template <class Cfg> static GemmLaunch built_for(GemmKernel fn) { return GemmLaunch{fn, Cfg::BM, Cfg::BN}; }
// THE place where the layout flags become template arguments: f(A k-contiguous, B k-contiguous)
template <class F> static GemmKernel by_layout(const GemmRoute& r, F f) {
    return by_flag(r.akc, [&](auto ak) { return by_flag(r.bkc, [&](auto bk) { return f(ak, bk); }); });
}

using Cfg64 = TileCfg<2, 2, 1, 1>; using Cfg128x32 = TileCfg<4, 1, 1, 1>; using Cfg32x128 = TileCfg<1, 4, 1, 1>; using Cfg64x128 = TileCfg<2, 2, 1, 2>;
using Cfg256x128 = TileCfg<2, 2, 4, 2>;
using Cfg128x256 = TileCfg<2, 2, 2, 4>; using Cfg64x256 = TileCfg<2, 2, 1, 4>; using Cfg96x256 = TileCfg<1, 4, 3, 2>; using Cfg256x96 = TileCfg<4, 1, 2, 3>;      // few output channels x many positions (backbone pointwise convolutions)

template <class Cfg> static GemmLaunch f32_tile(const GemmRoute& r) {
    return built_for<Cfg>(by_layout(r, [](auto ak, auto bk) -> GemmKernel { return gemm_f32_kernel<Cfg, decltype(ak)::value, decltype(bk)::value, true, SEGX_EPI_NONE>; }));
}
// the fused swish: k-contiguous A, row-contiguous B (segx_gemm_f32 refuses other layouts)
template <class Cfg, int E = SEGX_EPI_SWISH> static GemmLaunch f32_swish_tile() { return built_for<Cfg>(gemm_f32_kernel<Cfg, true, false, true, E>); }
// ... and the fused ReLU, the same set of forms
template <int E> static GemmLaunch f32_act_kernel(const GemmRoute& r) {
    if (!r.vec) return built_for<Cfg128>(gemm_f32_kernel<Cfg128, true, false, false, E>);
    return r.tile == SEGX_TILE_64x64 ? f32_swish_tile<Cfg64, E>() : r.tile == SEGX_TILE_64x128 ? f32_swish_tile<Cfg64x128, E>() : f32_swish_tile<Cfg128, E>();
}
static GemmLaunch f32_kernel(const GemmRoute& r) {
    if (r.epi == SEGX_EPI_SWISH) return f32_act_kernel<SEGX_EPI_SWISH>(r);
    if (r.epi == SEGX_EPI_RELU) return f32_act_kernel<SEGX_EPI_RELU>(r);
    if (r.epi == SEGX_EPI_GELU)
        return built_for<Cfg128>(by_flag(r.bkc, [&](auto bk) { return by_flag(r.vec, [](auto v) -> GemmKernel {
            return gemm_f32_kernel<Cfg128, true, decltype(bk)::value, decltype(v)::value, SEGX_EPI_GELU>; }); }));
    if (!r.vec) return built_for<Cfg128>(by_layout(r, [](auto ak, auto bk) -> GemmKernel { return gemm_f32_kernel<Cfg128, decltype(ak)::value, decltype(bk)::value, false, SEGX_EPI_NONE>; }));
    switch (r.tile) {
        case SEGX_TILE_64x64: return f32_tile<Cfg64>(r);
        case SEGX_TILE_128x32: return f32_tile<Cfg128x32>(r);
        case SEGX_TILE_32x128: return f32_tile<Cfg32x128>(r);
        case SEGX_TILE_64x128: return f32_tile<Cfg64x128>(r);
        default: return f32_tile<Cfg128>(r);
    }
}

// the four-wave bf16x6 kernels; W = waves per SIMD the tile's registers and LDS allow
template <bool LEAN, class Cfg, bool AK, bool BK, int E, int W, int T = 6> static GemmKernel x6_form() {
    if constexpr (LEAN) return gemm_x6_lean_kernel<Cfg, AK, BK, E, W, T>; else return gemm_x6_kernel<Cfg, AK, BK, E, W, 0, T>;
}
template <bool LEAN, class Cfg, int W> static GemmLaunch x6_tile(const GemmRoute& r) {
    return built_for<Cfg>(by_layout(r, [](auto ak, auto bk) { return x6_form<LEAN, Cfg, decltype(ak)::value, decltype(bk)::value, SEGX_EPI_NONE, W>(); }));
}
// the fused swish / ReLU: k-contiguous A, row-contiguous B, the three four-wave tiles
template <bool LEAN, int E> static GemmLaunch x6_act_kernel(const GemmRoute& r) {
    switch (r.tile) {
        case SEGX_TILE_64x64: return built_for<Cfg64>(x6_form<LEAN, Cfg64, true, false, E, 5>());
        case SEGX_TILE_64x128: return built_for<Cfg64x128>(x6_form<LEAN, Cfg64x128, true, false, E, 4>());
        default: return built_for<Cfg128>(x6_form<LEAN, Cfg128, true, false, E, 3>());
    }
}
template <bool LEAN> static GemmLaunch x6_kernel(const GemmRoute& r) {
    if (r.epi == SEGX_EPI_GELU) return built_for<Cfg128>(by_flag(r.bkc, [](auto bk) { return x6_form<LEAN, Cfg128, true, decltype(bk)::value, SEGX_EPI_GELU, 3>(); }));
    if (r.epi == SEGX_EPI_SWISH) return x6_act_kernel<LEAN, SEGX_EPI_SWISH>(r);
    if (r.epi == SEGX_EPI_RELU) return x6_act_kernel<LEAN, SEGX_EPI_RELU>(r);
    switch (r.tile) {
        case SEGX_TILE_64x64: return x6_tile<LEAN, Cfg64, 5>(r);
        case SEGX_TILE_64x128: return x6_tile<LEAN, Cfg64x128, 4>(r);
        default: return x6_tile<LEAN, Cfg128, 3>(r);
    }
}
// the three-term forms of the same kernels (exactly what x3_built() names), at the waves per SIMD of their six-term siblings
template <bool LEAN, class Cfg, int W> static GemmLaunch x3_tile(const GemmRoute& r) {
    if (r.epi == SEGX_EPI_SWISH) return built_for<Cfg>(x6_form<LEAN, Cfg, true, false, SEGX_EPI_SWISH, W, 3>());
    if (r.epi == SEGX_EPI_RELU) return built_for<Cfg>(x6_form<LEAN, Cfg, true, false, SEGX_EPI_RELU, W, 3>());
    if constexpr (LEAN) {
        if (r.bkc) return built_for<Cfg>(by_flag(r.akc, [](auto ak) { return x6_form<true, Cfg, decltype(ak)::value, true, SEGX_EPI_NONE, W, 3>(); }));
    }
    return built_for<Cfg>(x6_form<LEAN, Cfg, true, false, SEGX_EPI_NONE, W, 3>());
}
template <bool LEAN> static GemmLaunch x3_kernel(const GemmRoute& r) {
    if constexpr (LEAN) {
        if (r.epi == SEGX_EPI_GELU) return built_for<Cfg128>(by_flag(r.bkc, [](auto bk) { return x6_form<true, Cfg128, true, decltype(bk)::value, SEGX_EPI_GELU, 3, 3>(); }));
    }
    switch (r.tile) {
        case SEGX_TILE_64x64: return x3_tile<LEAN, Cfg64, 5>(r);
        case SEGX_TILE_64x128: return x3_tile<LEAN, Cfg64x128, 4>(r);
        default: return x3_tile<LEAN, Cfg128, 3>(r);
    }
}
// the schedule variants of gemm_x6_kernel (plain NT, default tile): <waves per SIMD, VAR>
template <int W, int VAR> static GemmLaunch x6_sched() { return built_for<Cfg128>(gemm_x6_kernel<Cfg128, true, true, SEGX_EPI_NONE, W, VAR>); }
static GemmLaunch x6_sched_kernel(int sched) {
    switch (sched) {
        case 1: return x6_sched<3, 1>();
        case 6: return x6_sched<2, 6>();
#ifdef SEGX_BENCH
        case 2: return x6_sched<3, 2>(); case 3: return x6_sched<3, 3>(); case 4: return x6_sched<3, 4>(); case 5: return x6_sched<3, 5>();
#endif
        default: return x6_sched<2, 0>();      // 7: the product schedule at two waves per SIMD (what the split-early schedule is compared with)
    }
}
template <class Cfg, bool AK, bool BK, int E> static GemmKernel ws_form(int sched) {
    constexpr bool NT = E == SEGX_EPI_NONE && AK && BK;      // the ablations are built for the plain NT form
    switch (sched) {
        case 1: return gemm_x6ws_kernel<Cfg, AK, BK, E, 1>;
#ifdef SEGX_BENCH
        case 2: return gemm_x6ws_kernel<Cfg, AK, BK, E, NT ? 2 : 0>; case 3: return gemm_x6ws_kernel<Cfg, AK, BK, E, NT ? 3 : 0>;
        case 4: return gemm_x6ws_kernel<Cfg, AK, BK, E, NT ? 4 : 0>; case 5: return gemm_x6ws_kernel<Cfg, AK, BK, E, NT ? 5 : 0>;
#endif
        default: return gemm_x6ws_kernel<Cfg, AK, BK, E, 0>;
    }
}
// every layout, and the fused GELU with a k-contiguous A (gemm_route names the GELU form for the 256 x 128 and 128 x 128 tiles only)
template <class Cfg> static GemmLaunch ws_tile(const GemmRoute& r) {
    if (r.epi == SEGX_EPI_GELU) return built_for<Cfg>(by_flag(r.bkc, [&](auto bk) { return ws_form<Cfg, true, decltype(bk)::value, SEGX_EPI_GELU>(r.sched); }));
    return built_for<Cfg>(by_layout(r, [&](auto ak, auto bk) { return ws_form<Cfg, decltype(ak)::value, decltype(bk)::value, SEGX_EPI_NONE>(r.sched); }));
}
static GemmLaunch ws_kernel(const GemmRoute& r) {
    switch (r.tile) {
        case SEGX_TILE_256x128: return ws_tile<Cfg256x128>(r);
        case SEGX_TILE_WS128x128: return ws_tile<Cfg128>(r);
        case SEGX_TILE_WS128x256: return ws_tile<Cfg128x256>(r);
        case SEGX_TILE_WS64x256: return ws_tile<Cfg64x256>(r);
        case SEGX_TILE_WS96x256: return built_for<Cfg96x256>(by_flag(r.bkc, [&](auto bk) { return ws_form<Cfg96x256, true, decltype(bk)::value, SEGX_EPI_NONE>(r.sched); }));
        default: return built_for<Cfg256x96>(by_flag(r.akc, [&](auto ak) { return ws_form<Cfg256x96, decltype(ak)::value, true, SEGX_EPI_NONE>(r.sched); }));
    }
}
template <class Cfg> static GemmLaunch ws3_tile(const GemmRoute& r) {
    return built_for<Cfg>(by_flag(r.bkc, [](auto bk) -> GemmKernel { return gemm_x6ws_kernel<Cfg, true, decltype(bk)::value, SEGX_EPI_NONE, 0, 3>; }));
}
static GemmLaunch ws3_kernel(const GemmRoute& r) {
    switch (r.tile) {
        case SEGX_TILE_256x128: return ws3_tile<Cfg256x128>(r);
        case SEGX_TILE_WS128x128: return ws3_tile<Cfg128>(r);
        case SEGX_TILE_WS128x256: return ws3_tile<Cfg128x256>(r);
        case SEGX_TILE_WS64x256: return built_for<Cfg64x256>(gemm_x6ws_kernel<Cfg64x256, true, false, SEGX_EPI_NONE, 0, 3>);
        case SEGX_TILE_WS96x256: return ws3_tile<Cfg96x256>(r);
        default: return built_for<Cfg256x96>(gemm_x6ws_kernel<Cfg256x96, true, true, SEGX_EPI_NONE, 0, 3>);
    }
}
template <class Cfg> static GemmLaunch ws_pre_tile(const GemmRoute& r) {
    return built_for<Cfg>(by_flag(r.akc, [](auto ak) -> GemmKernel { return gemm_x6ws_pre_kernel<Cfg, decltype(ak)::value>; }));
}
static GemmLaunch route_kernel(const GemmRoute& r) {
    if (r.terms == 3) {                                      // gemm_route set it for the forms x3_built() names only
        switch (r.family) {
            case GEMM_X6: return x3_kernel<false>(r);
#ifndef SEGX_NO_LEAN
            case GEMM_X6_LEAN: return x3_kernel<true>(r);
#endif
            default: return ws3_kernel(r);
        }
    }
    switch (r.family) {
        case GEMM_X6: return r.sched ? x6_sched_kernel(r.sched) : x6_kernel<false>(r);
#ifndef SEGX_NO_LEAN
        case GEMM_X6_LEAN: return x6_kernel<true>(r);
#endif
        case GEMM_WS: return ws_kernel(r);
        case GEMM_WS_PRE: return r.tile == SEGX_TILE_256x128 ? ws_pre_tile<Cfg256x128>(r) : ws_pre_tile<Cfg128x256>(r);
        default: return f32_kernel(r);
    }
}
static void set_tiles(GemmArgs& g, const GemmLaunch& k, const GemmRoute& r) {
    g.tiles_m = ceil_div(g.M, k.bm); g.tiles_n = ceil_div(g.N, k.bn); g.mfast = r.walk ? tile_walk(g.M, g.N, g.K, g.tiles_m) : 0;
}
// persistent launch: one workgroup per CU, a multiple of eight (one run of items per XCD and round)
static int persistent_grid(const GemmArgs& g, const GemmRoute& r, int* grid) {
    const int64_t items = (int64_t)g.tiles_m * g.tiles_n * g.nbatch * g.splitk;
    SEGX_REQUIRE(items < 2147483647LL - 512, "segx_gemm_f32: too many tiles");
    *grid = (int)i64min(r.ws_grid, (items + 7) / 8 * 8);
    return 0;
}
// The workspace holds nslabs slabs of M x N (slab (zk, zb) at (zk * nbatch + zb) * M * N): one deterministic sum over all of them.  The streaming skinny kernel's
// slabs are always few outputs (one side <= 32 rows): it takes one of the two per-output-parts forms whatever the sizes.
static void slab_reduce(const segx_gemm_desc* d, float* C, const float* bias, int nslabs, bool skinny, hipStream_t stream) {
    const int64_t total = (int64_t)d->M * d->N;
    const float* ws = static_cast<const float*>(d->workspace);
    if (total * 16 <= 512 * 1024 && nslabs >= 16)          // few outputs, many slabs: 16 threads per output
        hipLaunchKernelGGL((slab_sum_parts_kernel<16>), dim3((unsigned)((total + 15) / 16)), dim3(256), 0, stream, ws, C, bias, d->M, d->N, nslabs, total, d->c_m, d->alpha, d->bias_mode);
    else if (skinny || (total * 4 <= 1024 * 1024 && nslabs >= 4))
        hipLaunchKernelGGL((slab_sum_parts_kernel<4>), dim3((unsigned)((total + 63) / 64)), dim3(256), 0, stream, ws, C, bias, d->M, d->N, nslabs, total, d->c_m, d->alpha, d->bias_mode);
    else
        SEGX_SPLITK_REDUCE((unsigned)i64min(2048, (total + 255) / 256), stream, ws, C, bias, d->M, d->N, 1, nslabs, total, (int64_t)0, (int64_t)0, d->c_m, d->alpha,
                           d->bias_mode, (int64_t)0, (int64_t)0, total, (const float*)nullptr);
}
}  // namespace segx

extern "C" int segx_gemm_plan(const float* A, const float* B, const segx_gemm_desc* d, int* tile, int* splitk) { return segx::gemm_plan_impl(A, B, d, tile, splitk, true); }
// the cost model's own pick, without the measured table (tools/tune_gemm.py compares every candidate with it to decide which shapes need a table entry)
extern "C" int segx_gemm_plan_model(const float* A, const float* B, const segx_gemm_desc* d, int* tile, int* splitk) { return segx::gemm_plan_impl(A, B, d, tile, splitk, false); }

// the route segx_gemm_f32 would take for this descriptor under the knobs as they are now; launches nothing
extern "C" int segx_gemm_route(const float* A, const float* B, const segx_gemm_desc* d, int32_t* out) {
    using namespace segx;
    SEGX_REQUIRE(A && B && d && out && d->M > 0 && d->N > 0 && d->K > 0 && d->nb0 > 0 && d->nb1 > 0, "segx_gemm_route: bad args");
    SEGX_REQUIRE(d->tile >= SEGX_TILE_AUTO && d->tile <= SEGX_TILE_SKINNY_NT && d->engine >= SEGX_ENGINE_SEL_DEFAULT && d->engine <= SEGX_ENGINE_SEL_BF16X6,
                 "segx_gemm_route: bad tile %d or engine selector %d", d->tile, d->engine);
    GemmRoute r;
    const int rc = gemm_route(A, B, d, &r);
    if (rc) return rc;
    out[0] = r.family; out[1] = r.tile; out[2] = r.terms; out[3] = r.splitk;
    return 0;
}

extern "C" int segx_gemm_f32(const float* A, const float* B, float* C, const segx_gemm_desc* d, void* stream_) {
    using namespace segx;
    hipStream_t stream = (hipStream_t)stream_;
    SEGX_REQUIRE(A && B && C && d, "segx_gemm_f32: null pointer");
    SEGX_REQUIRE(d->M > 0 && d->N > 0 && d->K > 0 && d->nb0 > 0 && d->nb1 > 0, "segx_gemm_f32: bad sizes M=%d N=%d K=%d nb=%dx%d",
                 d->M, d->N, d->K, d->nb0, d->nb1);
    SEGX_REQUIRE(d->a_m == 1 || d->a_k == 1, "segx_gemm_f32: A needs a unit stride (a_m=%lld a_k=%lld)", (long long)d->a_m, (long long)d->a_k);
    SEGX_REQUIRE(d->b_n == 1 || d->b_k == 1, "segx_gemm_f32: B needs a unit stride (b_n=%lld b_k=%lld)", (long long)d->b_n, (long long)d->b_k);
    SEGX_REQUIRE(d->epilogue == SEGX_EPI_NONE || d->epilogue == SEGX_EPI_GELU || d->epilogue == SEGX_EPI_SWISH || d->epilogue == SEGX_EPI_RELU, "segx_gemm_f32: bad epilogue %d", d->epilogue);
    SEGX_REQUIRE(d->epilogue != SEGX_EPI_RELU || (d->a_k == 1 && d->b_n == 1 && d->b_k != 1 && !d->resid && !d->gmax && d->dropout_p == 0.f),
                 "segx_gemm_f32: the relu epilogue is built for a pointwise convolution's forward (A k-contiguous, B row-contiguous; no resid, gmax or dropout)");
    SEGX_REQUIRE(d->epilogue != SEGX_EPI_SWISH || (d->a_k == 1 && d->b_n == 1 && d->b_k != 1 && !d->resid && !d->gmax && d->dropout_p == 0.f),
                 "segx_gemm_f32: the swish epilogue is built for a pointwise convolution's forward (A k-contiguous, B row-contiguous; no resid, gmax or dropout)");
    SEGX_REQUIRE(d->epilogue != SEGX_EPI_GELU || d->aux, "segx_gemm_f32: GELU epilogue needs aux");
    SEGX_REQUIRE(d->bias_mode == SEGX_BIAS_NONE || d->bias, "segx_gemm_f32: bias_mode set but bias null");
    SEGX_REQUIRE(d->dropout_p >= 0.f && d->dropout_p < 1.f, "segx_gemm_f32: dropout_p out of range");
    const int splitk = d->splitk > 1 ? d->splitk : 1;
    SEGX_REQUIRE(splitk == 1 || (d->workspace && d->epilogue == SEGX_EPI_NONE && !d->gmax), "segx_gemm_f32: split-K needs workspace and a plain epilogue");
    const bool breduce = d->batch_reduce != 0;
    SEGX_REQUIRE(!breduce || (d->workspace && d->epilogue == SEGX_EPI_NONE && !d->gmax), "segx_gemm_f32: batch_reduce needs workspace and a plain epilogue");
    SEGX_REQUIRE(!d->resid || (d->epilogue == SEGX_EPI_NONE && !breduce && !d->gmax), "segx_gemm_f32: resid needs a plain epilogue (no GELU, no batch_reduce, no gmax)");
    SEGX_REQUIRE(d->tile >= SEGX_TILE_AUTO && d->tile <= SEGX_TILE_SKINNY_NT, "segx_gemm_f32: bad tile %d", d->tile);
    SEGX_REQUIRE(d->engine >= SEGX_ENGINE_SEL_DEFAULT && d->engine <= SEGX_ENGINE_SEL_BF16X6, "segx_gemm_f32: bad engine selector %d", d->engine);
    GemmRoute r;
    int rc = gemm_route(A, B, d, &r);
    if (rc) return rc;

    const int nbatch = d->nb0 * d->nb1;
    const float* bias = d->bias_mode ? d->bias : nullptr;
    if (r.family == GEMM_SKINNY) {
        const int nslabs = splitk * nbatch;
        rc = launch_skinny_nt(A, B, static_cast<float*>(d->workspace), d->M, d->N, d->K, d->nb0, d->nb1, d->a_b0, d->a_b1, d->a_m, d->b_b0, d->b_b1, d->b_n, nslabs, stream);
        if (rc) return rc;
        slab_reduce(d, C, bias, nslabs, true, stream);
        return check_launch("segx_gemm_f32/skinny_nt_reduce");
    }
    GemmArgs g;
    g.A = A; g.B = B; g.C = C; g.bias = bias; g.aux = d->epilogue == SEGX_EPI_GELU ? d->aux : nullptr;
    g.gmax = d->gmax;
    g.M = d->M; g.N = d->N; g.K = d->K; g.nb1 = d->nb1; g.nbatch = nbatch;
    g.a_b0 = d->a_b0; g.a_b1 = d->a_b1; g.a_m = d->a_m; g.a_k = d->a_k;
    g.b_b0 = d->b_b0; g.b_b1 = d->b_b1; g.b_n = d->b_n; g.b_k = d->b_k;
    g.c_b0 = d->c_b0; g.c_b1 = d->c_b1; g.c_m = d->c_m; g.bias_b1 = d->bias_b1; g.bias_b0 = d->bias_b0;
    g.alpha = d->alpha; g.epilogue = d->epilogue; g.bias_mode = d->bias_mode;
    g.vecA = r.vec; g.vecB = r.vec;
    g.dropout_p = d->dropout_p; g.seed = d->seed; g.offset = d->offset; g.rbase = rng_base();
    g.splitk = splitk;
    // k_chunk: multiple of the k-tile so slabs start on tile boundaries (and stay float4-aligned)
    g.k_chunk = splitk == 1 ? d->K : ceil_div(ceil_div(d->K, splitk), BKT) * BKT;
    g.c_split = (int64_t)nbatch * d->M * d->N;
    g.slab = breduce ? 1 : 0;
    g.Bp = nullptr; g.bp_plane = g.bp_b0 = g.bp_b1 = 0;
    if (r.family == GEMM_WS_PRE) { g.Bp = static_cast<const unsigned short*>(d->b_planes); g.bp_plane = (int64_t)d->N * d->K; g.bp_b0 = d->bp_b0; g.bp_b1 = d->bp_b1; }
    g.resid = d->resid;
    if (splitk > 1 || breduce) g.C = d->workspace;

    if (r.family != GEMM_F32) knobs().x6_launches.fetch_add(1, std::memory_order_relaxed);
    if (r.terms == 3) knobs().x3_launches.fetch_add(1, std::memory_order_relaxed);
    const GemmLaunch k = route_kernel(r);
    set_tiles(g, k, r);
    if (r.family == GEMM_WS || r.family == GEMM_WS_PRE) {
        int grid;
        rc = persistent_grid(g, r, &grid);
        if (rc) return rc;
        hipLaunchKernelGGL(k.fn, dim3(grid), dim3(512), 0, stream, g);
    } else
        hipLaunchKernelGGL(k.fn, dim3(g.tiles_m * g.tiles_n, nbatch, splitk), dim3(256), 0, stream, g);
    rc = check_launch("segx_gemm_f32");
    if (rc) return rc;
    if (breduce) {
        SEGX_REQUIRE((int64_t)splitk * nbatch < 2147483647LL, "segx_gemm_f32: too many slabs");
        slab_reduce(d, C, bias, splitk * nbatch, false, stream);
        return check_launch("segx_gemm_f32/batch_reduce");
    }
    if (splitk > 1) {
        const int64_t total = g.c_split;
        const int blocks = (int)i64min(2048, (total + 255) / 256);
        SEGX_SPLITK_REDUCE(blocks, stream, (const float*)d->workspace, C, g.bias, d->M, d->N, d->nb1, splitk, g.c_split, d->c_b0, d->c_b1, d->c_m, d->alpha, d->bias_mode, d->bias_b1, d->bias_b0,
                           total, (const float*)d->resid);
        rc = check_launch("segx_gemm_f32/splitk_reduce");
    }
    return rc;
}

extern "C" int64_t segx_x6_presplit_elems(int rows, int K, int nb0, int nb1) { return (int64_t)nb0 * nb1 * 3 * rows * K; }

extern "C" int segx_x6_presplit(const float* W, int rows, int K, int64_t s_row, int64_t s_k, int nb0, int nb1, int64_t s_b0, int64_t s_b1, void* planes,
                                void* stream_) {
    using namespace segx;
    SEGX_REQUIRE(W && planes, "segx_x6_presplit: null pointer");
    SEGX_REQUIRE(rows > 0 && K > 0 && K % 8 == 0 && nb0 > 0 && nb1 > 0, "segx_x6_presplit: rows=%d K=%d (a multiple of 8) nb=%dx%d", rows, K, nb0, nb1);
    SEGX_REQUIRE(s_row == 1 || s_k == 1, "segx_x6_presplit: the operand needs a unit stride (s_row=%lld s_k=%lld)", (long long)s_row, (long long)s_k);
    SEGX_REQUIRE((reinterpret_cast<uintptr_t>(planes) & 15) == 0, "segx_x6_presplit: planes must be 16-byte aligned");
    const int64_t per_batch = (int64_t)rows * K;
    const int64_t blocks = (per_batch / 8 + 255) / 256;
    hipLaunchKernelGGL(x6_presplit_kernel, dim3((unsigned)i64min(blocks, 65536), nb0 * nb1), dim3(256), 0, (hipStream_t)stream_, W,
                       static_cast<unsigned short*>(planes), rows, K, s_row, s_k, nb1, s_b0, s_b1, per_batch);
    return check_launch("segx_x6_presplit");
}
