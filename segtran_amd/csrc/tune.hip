// tune.hip -- segx_tune / segx_tune_get: the process-wide knobs, generated from SEGX_KNOB_TABLE (common.h), which also states the special cases.
#include "common.h"

extern "C" int segx_tune(int knob, int value) {
    segx::Knobs& k = segx::knobs();
    if (knob == 5) return k.x6_launches.exchange(0);                                              // the launch counter: read and reset
    if (knob == 9 && value % 8) return -1;
    if (knob == 20 && value != 6 && value != 3) return -1;
#ifndef SEGX_BENCH
    if (knob == 6 && value >= 2 && value <= 5) return -1;                                         // ablations whose results are NOT the GEMM
#endif
    switch (knob) {
#define SEGX_KNOB_SET(id, field, def, lo, hi) case id: { if (value < (lo) || value > (hi)) return -1; const int prev = k.field.exchange(value); return id == 4 ? prev : 0; }
        SEGX_KNOB_TABLE(SEGX_KNOB_SET)
#undef SEGX_KNOB_SET
        default: return -1;
    }
}
extern "C" int segx_tune_get(int knob) {
    const segx::Knobs& k = segx::knobs();
    switch (knob) {
#define SEGX_KNOB_GET(id, field, def, lo, hi) case id: return segx::kget(k.field);
        SEGX_KNOB_TABLE(SEGX_KNOB_GET)
#undef SEGX_KNOB_GET
        default: return -1;
    }
}
extern "C" int segx_x3_launches(void) { return segx::knobs().x3_launches.exchange(0); }         // read and reset, like knob 5
