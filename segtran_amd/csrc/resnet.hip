// resnet.hip -- the closing operation of a ResNet block: y = relu((z + bias[plane % C]) + r), and its backward dz = y > 0 ? dy : 0.
// z is what the block's last BatchNorm wrote (training: the skip is already added there, r = NULL) or what its last convolution wrote with the BatchNorm folded
// into the filters (inference: r = the shortcut, bias = the folded shifts of the block's last and down-sample BatchNorms).
// Pure HBM streams: every element is read once and written once, 16 bytes per lane where the operands allow it, and no integer division per element.
#include "common.h"

namespace segx {

constexpr int AR_THREADS = 256;
constexpr int AR_UNROLL = 4;            // float4 elements a thread of the flat kernels has in flight: all loads of a round are issued before the first store
constexpr int AR_FLAT_CAP = 1024;       // workgroups of a flat launch (4 per CU, 16 KB in flight per workgroup and operand); the grid-stride loop reaches the rest
constexpr int AR_GRID_CAP = 2048;       // workgroups of a bias launch
constexpr int AR_RUN = 512;             // elements (float4 or float) of one run of planes in the bias kernels: two per thread
// One sweep of a full grid covers AR_FLAT_CAP * AR_THREADS * AR_UNROLL float4 = 4,194,304 floats in the flat kernels and AR_GRID_CAP runs of at most AR_RUN float4
// (4,194,304 floats) in the bias kernels: tests/test_resnet_kernels.py runs one shape beyond both.

// torch.relu: NaN stays NaN (a comparison with NaN is false, so v itself is returned); fmaxf(v, 0) would return 0
__device__ __forceinline__ float relu_keep_nan(float v) { return v < 0.f ? 0.f : v; }

// ---- no bias: the tensor is one flat array.  n4 float4 elements (0 where a pointer is not 16-byte aligned), then the scalar remainder up to n ----
template <bool HAS_R>
__global__ __launch_bounds__(AR_THREADS) void add_relu_flat_kernel(const float* Z, const float* R, float* Y, int64_t n4, int64_t n) {
    const int64_t stride = (int64_t)gridDim.x * AR_THREADS, first = (int64_t)blockIdx.x * AR_THREADS + threadIdx.x;
    const float4* z4 = reinterpret_cast<const float4*>(Z);
    const float4* r4 = reinterpret_cast<const float4*>(R);
    float4* y4 = reinterpret_cast<float4*>(Y);
    for (int64_t i = first; i < n4; i += stride * AR_UNROLL) {                      // Y may alias Z: an element is read before it is written, by the same thread
        float4 v[AR_UNROLL], r[AR_UNROLL];
#pragma unroll
        for (int u = 0; u < AR_UNROLL; ++u) {
            const int64_t j = i + u * stride;
            if (j < n4) { v[u] = z4[j]; if (HAS_R) r[u] = r4[j]; }
        }
#pragma unroll
        for (int u = 0; u < AR_UNROLL; ++u) {
            const int64_t j = i + u * stride;
            if (j < n4) {
                float4 t = v[u];
                if (HAS_R) { t.x += r[u].x; t.y += r[u].y; t.z += r[u].z; t.w += r[u].w; }
                t.x = relu_keep_nan(t.x); t.y = relu_keep_nan(t.y); t.z = relu_keep_nan(t.z); t.w = relu_keep_nan(t.w);
                y4[j] = t;
            }
        }
    }
    for (int64_t i = n4 * 4 + first; i < n; i += stride) {
        float v = Z[i];
        if (HAS_R) v += R[i];
        Y[i] = relu_keep_nan(v);
    }
}

// dz = y > 0 ? dy : 0 (torch's threshold_backward: 0 at y == 0, and dy itself -- NaN included -- where y > 0)
__global__ __launch_bounds__(AR_THREADS) void add_relu_bwd_kernel(const float* __restrict__ dY, const float* __restrict__ Y, float* __restrict__ dZ, int64_t n4, int64_t n) {
    const int64_t stride = (int64_t)gridDim.x * AR_THREADS, first = (int64_t)blockIdx.x * AR_THREADS + threadIdx.x;
    const float4* y4 = reinterpret_cast<const float4*>(Y);
    const float4* g4 = reinterpret_cast<const float4*>(dY);
    float4* d4 = reinterpret_cast<float4*>(dZ);
    for (int64_t i = first; i < n4; i += stride * AR_UNROLL) {
        float4 y[AR_UNROLL], g[AR_UNROLL];
#pragma unroll
        for (int u = 0; u < AR_UNROLL; ++u) {
            const int64_t j = i + u * stride;
            if (j < n4) { y[u] = y4[j]; g[u] = g4[j]; }
        }
#pragma unroll
        for (int u = 0; u < AR_UNROLL; ++u) {
            const int64_t j = i + u * stride;
            if (j < n4) d4[j] = make_float4(y[u].x > 0.f ? g[u].x : 0.f, y[u].y > 0.f ? g[u].y : 0.f, y[u].z > 0.f ? g[u].z : 0.f, y[u].w > 0.f ? g[u].w : 0.f);
        }
    }
    for (int64_t i = n4 * 4 + first; i < n; i += stride) dZ[i] = Y[i] > 0.f ? dY[i] : 0.f;
}

// ---- with a bias: planes of SV elements (V floats each).  A workgroup row (blockIdx.y, grid-stride) takes a RUN of P consecutive planes, the workgroups of the row
// (blockIdx.x) share the run's P * SV elements.  A thread finds its (plane, offset) once -- the same in every run, since a run starts on a plane -- and then walks by
// the launch's step, which the host has split into whole planes and a rest: additions and one conditional subtraction per element, no division.  The channel of the
// run's first plane costs one multiply-high per thread and run (FastDiv).
template <int V> struct ArVec { typedef float type; };
template <> struct ArVec<4> { typedef float4 type; };
__device__ __forceinline__ float ar_one(float z, float b, float r) { return relu_keep_nan((z + b) + r); }
__device__ __forceinline__ float ar_one(float z, float b) { return relu_keep_nan(z + b); }
template <bool HAS_R> __device__ __forceinline__ float ar_elem(float z, float b, const float* R, int64_t at) { return HAS_R ? ar_one(z, b, R[at]) : ar_one(z, b); }
template <bool HAS_R> __device__ __forceinline__ float4 ar_elem(float4 z, float b, const float4* R, int64_t at) {
    if (HAS_R) {
        const float4 r = R[at];
        return make_float4(ar_one(z.x, b, r.x), ar_one(z.y, b, r.y), ar_one(z.z, b, r.z), ar_one(z.w, b, r.w));
    }
    return make_float4(ar_one(z.x, b), ar_one(z.y, b), ar_one(z.z, b), ar_one(z.w, b));
}

struct ArWalk { int step_p, step_o, step_c; };      // host-side split of the launch's step gridDim.x * AR_THREADS = step_p * SV + step_o; step_c = step_p % C

template <int V, bool HAS_R>
__global__ __launch_bounds__(AR_THREADS) void add_relu_bias_kernel(const float* Z, const float* R, const float* __restrict__ bias, float* Y, int64_t planes, int C,
                                                                   FastDiv divC, int SV, int P, FastDiv divSV, ArWalk w) {
    typedef typename ArVec<V>::type T;
    const T* z = reinterpret_cast<const T*>(Z);
    const T* r = reinterpret_cast<const T*>(R);
    T* y = reinterpret_cast<T*>(Y);
    // this thread's first element of a run: plane p_first, offset o_first (one division per thread and launch)
    const int e0 = (int)blockIdx.x * AR_THREADS + (int)threadIdx.x;
    const int p_first = fdiv(e0, divSV), o_first = e0 - p_first * SV;
    const int64_t nruns = (planes + P - 1) / P;
    for (int64_t run = blockIdx.y; run < nruns; run += gridDim.y) {
        const int64_t plane0 = run * P;
        const int np = (int)i64min((int64_t)P, planes - plane0);
        int p = p_first, o = o_first;
        if (p >= np) continue;
        const int g = (int)plane0 + p;                                              // planes < 2^31 (host check)
        int c = g - fdiv(g, divC) * C;
        const T* zr = z + plane0 * SV; T* yr = y + plane0 * SV;
        const T* rr = HAS_R ? r + plane0 * SV : nullptr;
        while (p < np) {
            const int64_t at = (int64_t)p * SV + o;
            yr[at] = ar_elem<HAS_R>(zr[at], bias[c], rr, at);
            p += w.step_p; o += w.step_o; c += w.step_c;
            if (o >= SV) { o -= SV; ++p; ++c; }
            if (c >= C) c -= C;
        }
    }
}

template <int V, bool HAS_R>
static void launch_bias(const float* Z, const float* R, const float* bias, float* Y, int64_t planes, int C, int64_t SV, hipStream_t stream) {
    // a run: P whole planes of at most AR_RUN elements together, or one plane shared by gx workgroups
    const int P = SV >= AR_RUN ? 1 : (int)(AR_RUN / SV);
    const int64_t run_elems = (int64_t)P * SV;
    int gx = (int)i64min((run_elems + 2 * AR_THREADS - 1) / (2 * AR_THREADS), 64);
    if (gx < 1) gx = 1;
    const int64_t nruns = (planes + P - 1) / P;
    const int gy = (int)i64max(1, i64min(nruns, AR_GRID_CAP / gx));
    const int step = gx * AR_THREADS;
    ArWalk w;
    w.step_p = (int)(step / SV); w.step_o = (int)(step % SV); w.step_c = w.step_p % C;
    hipLaunchKernelGGL((add_relu_bias_kernel<V, HAS_R>), dim3(gx, gy), dim3(AR_THREADS), 0, stream, Z, R, bias, Y, planes, C, make_fastdiv(C), (int)SV, P,
                       make_fastdiv((int)SV), w);
}

static inline bool ar_aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
static inline int ar_flat_grid(int64_t n4, int64_t n) {
    const int64_t per = n4 > 0 ? (int64_t)AR_THREADS * AR_UNROLL : AR_THREADS, work = n4 > 0 ? n4 : n;
    return (int)i64max(1, i64min((work + per - 1) / per, AR_FLAT_CAP));
}

}  // namespace segx

using namespace segx;
#define SEGX_STREAM hipStream_t stream = (hipStream_t)stream_

extern "C" int segx_add_relu_fwd(const float* Z, const float* R, const float* bias, float* Y, int64_t planes, int C, int64_t S, void* stream_) {
    SEGX_STREAM;
    SEGX_REQUIRE(Z && Y && planes > 0 && S > 0, "segx_add_relu_fwd: bad args (Z, Y non-null; planes, S > 0)");
    SEGX_REQUIRE(planes <= INT64_MAX / S, "segx_add_relu_fwd: planes * S overflows");
    const int64_t n = planes * S;
    const bool vec = ar_aligned16(Z) && ar_aligned16(Y) && (!R || ar_aligned16(R));
    if (!bias) {
        const int64_t n4 = vec ? n / 4 : 0;
        const int grid = ar_flat_grid(n4, n);
        if (R) hipLaunchKernelGGL(add_relu_flat_kernel<true>, dim3(grid), dim3(AR_THREADS), 0, stream, Z, R, Y, n4, n);
        else hipLaunchKernelGGL(add_relu_flat_kernel<false>, dim3(grid), dim3(AR_THREADS), 0, stream, Z, R, Y, n4, n);
        return check_launch("segx_add_relu_fwd");
    }
    SEGX_REQUIRE(C > 0 && planes % C == 0, "segx_add_relu_fwd: with a bias, planes must be a multiple of C > 0 (got planes %lld, C %d)", (long long)planes, C);
    SEGX_REQUIRE(planes < (1ll << 31) - AR_RUN && S < (1ll << 31), "segx_add_relu_fwd: with a bias, planes and S must stay below 2^31");
    if (vec && S % 4 == 0) {
        if (R) launch_bias<4, true>(Z, R, bias, Y, planes, C, S / 4, stream);
        else launch_bias<4, false>(Z, R, bias, Y, planes, C, S / 4, stream);
    } else {
        if (R) launch_bias<1, true>(Z, R, bias, Y, planes, C, S, stream);
        else launch_bias<1, false>(Z, R, bias, Y, planes, C, S, stream);
    }
    return check_launch("segx_add_relu_fwd");
}

extern "C" int segx_add_relu_bwd(const float* dY, const float* Y, float* dZ, int64_t planes, int64_t S, void* stream_) {
    SEGX_STREAM;
    SEGX_REQUIRE(dY && Y && dZ && planes > 0 && S > 0, "segx_add_relu_bwd: bad args (dY, Y, dZ non-null; planes, S > 0)");
    SEGX_REQUIRE(planes <= INT64_MAX / S, "segx_add_relu_bwd: planes * S overflows");
    SEGX_REQUIRE(dZ != Y, "segx_add_relu_bwd: dZ must not alias Y");
    const int64_t n = planes * S;
    const int64_t n4 = ar_aligned16(dY) && ar_aligned16(Y) && ar_aligned16(dZ) ? n / 4 : 0;
    hipLaunchKernelGGL(add_relu_bwd_kernel, dim3(ar_flat_grid(n4, n)), dim3(AR_THREADS), 0, stream, dY, Y, dZ, n4, n);
    return check_launch("segx_add_relu_bwd");
}
