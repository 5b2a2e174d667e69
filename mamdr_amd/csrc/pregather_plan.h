// Slice planner of the riders in k_wgrad_adam (fused_kernels.hip): which positions of the window announced by
// mamdr_pregather_ahead one launch gathers.  Host code without HIP dependencies (tests/test_pregather_plan_host.py builds it
// with the host compiler alone).
//
// A window is a list of passes.  Pass k of n rows owns n + PREP_PAD positions -- its rows, then the zero padding rows that
// carry its domain -- and an empty pass owns none (it has no steps).  The cursor (pass, pos) is the first position nobody
// gathered yet.  A slice is at most two segments of consecutive positions, each inside one pass: it ends early at a pass
// boundary rather than span a third pass.
#pragma once

#include <cstdint>

namespace mamdr {

constexpr int PREP_PAD = 16;          // padding rows behind every pass of the pass buffer (see pass_prep_row)

struct PrePlanCursor {
    int pass = 0;
    int64_t pos = 0;
};
struct PrePlanSeg {
    int pass = 0;
    int64_t first = 0, count = 0;     // positions [first, first + count) of the pass, in [0, rows + PREP_PAD)
};
struct PrePlanSlice {
    int n_seg = 0;
    PrePlanSeg seg[2];
    int64_t count() const { return seg[0].count + seg[1].count; }
};

inline int64_t pre_plan_positions(int64_t rows) { return rows > 0 ? rows + PREP_PAD : 0; }

// the cursor moved past passes without positions left; pass == n_pass: the window is done
inline void pre_plan_settle(const int64_t* pass_rows, int n_pass, PrePlanCursor& cur) {
    while (cur.pass < n_pass && cur.pos >= pre_plan_positions(pass_rows[cur.pass])) {
        cur.pass += 1;
        cur.pos = 0;
    }
}

// the next slice of at most `quota` positions; advances the cursor
inline PrePlanSlice pre_plan_next(const int64_t* pass_rows, int n_pass, PrePlanCursor& cur, int64_t quota) {
    PrePlanSlice s;
    while (s.n_seg < 2 && quota > 0) {
        pre_plan_settle(pass_rows, n_pass, cur);
        if (cur.pass >= n_pass) break;
        const int64_t left = pre_plan_positions(pass_rows[cur.pass]) - cur.pos;
        PrePlanSeg& g = s.seg[s.n_seg++];
        g.pass = cur.pass;
        g.first = cur.pos;
        g.count = left < quota ? left : quota;
        cur.pos += g.count;
        quota -= g.count;
    }
    pre_plan_settle(pass_rows, n_pass, cur);
    return s;
}

}  // namespace mamdr
