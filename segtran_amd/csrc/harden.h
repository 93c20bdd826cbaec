// harden.h -- the n-hot hardening of one cell (datasets2d.py:178-196, datasets3d.py:92-111), shared by the sliding-window kernels (infer.hip) and the n-hot
// evaluation tail (metrics.hip): the same inline function, hence the same maps.
#pragma once
#include "common.h"

namespace segx {

// One cell's C soft values p[] -> soft / hard planes (both already offset to the cell of class 0; classes lie S floats apart).  mode 1 first makes a BraTS
// prediction consistent, the permissive way (is_conservative=False): P(WT) = max(P(ET), P(WT), P(TC)), P(TC) = max(P(ET), P(TC));  then
// hard[c >= 1] = soft[c] >= T and hard[0] = (no other class is on).  harden_kernel, window_merge_kernel and nhot_case_tail_kernel call it.
// MAXC: the compile-time class bound (8 or 16, C <= MAXC).  Every loop over the classes runs MAXC trips under a `c < C` predicate, so p[] is indexed by constants
// only and stays in registers (an array indexed by a run-time class count goes to scratch at 16 entries); the C <= 8 calls run the 8 form and keep its registers.
template <int MAXC>
__device__ __forceinline__ void harden_cell(float* p, int C, int mode, float T, float* __restrict__ soft, float* __restrict__ hard, int64_t S) {
    if (mode == 1) {                                   // C == 4: [bg, ET, WT, TC]
        const float et = p[1], wt = p[2], tc = p[3];
        p[2] = fmaxf(fmaxf(et, wt), tc);
        p[3] = fmaxf(et, tc);
    }
    bool any = false;
#pragma unroll
    for (int c = 1; c < MAXC; ++c) {
        if (c < C) {
            const bool on = p[c] >= T;
            any = any || on;
            hard[c * S] = on ? 1.0f : 0.0f;
            if (soft) soft[c * S] = p[c];
        }
    }
    hard[0] = any ? 0.0f : 1.0f;
    if (soft) soft[0] = p[0];
}

}  // namespace segx
