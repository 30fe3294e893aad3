// pose_solve_dev.h -- the 6 x 6 solve of an LM step of the intra-camera pose solve (pose.hip), lane-parallel on one wave.
#pragma once

#include "cs_common.h"

#pragma clang fp contract(off)   // a multiply, then a subtract: the solve's bits are the entry-per-lane form's

#ifdef __HIPCC__

// (A + lambda I) p = B by Gauss-Jordan elimination with partial pivoting on [A | B] (the reference forms the LAPACK inverse and
// multiplies: same solution), ONE COLUMN PER LANE: lane j < 7 holds M[0..5][j] in col[0..5] (column 6 = B); lanes >= 7 carry
// nothing that is read.  Every lane of a wave running all 42 entries' arithmetic redundantly cost ~800 wave instructions per LM
// step, issued at 4 cycles each -- a third of the step; here a pivot step is one divide and five multiply-subtracts across the
// lanes, and nothing is gathered from lane to lane: the pivot search runs on lane c's own registers and its row index leaves
// through one v_readlane, the row swap is a swap of two registers under a wave-uniform condition, the pivot and the five factors
// (column c, all in lane c) leave through v_readlane pairs and come back as uniform operands.  No exchange goes through LDS.
// Element for element the same operations as the register version: the pivot of column c is the first row >= c with the
// largest |M[r][c]|, the pivot row is divided by it, every other row loses f times the pivot row (a multiply, then a subtract:
// contraction is off), columns <= c are left as they are.
// which of the 28 sums (upper triangle of A row by row, then B) is M[r][j]
__device__ __forceinline__ int solve66_entry(int r, int j) {
    if (j >= 6) return 21 + r;
    const int a = r < j ? r : j, b = r < j ? j : r;
    return a * 6 - (a * (a - 1)) / 2 + (b - a);
}
__device__ __forceinline__ void solve66_lanes(double (&col)[6], int lane, double* param) {
    const int j = lane;
#pragma unroll
    for (int c = 0; c < 6; ++c) {
        double best = fabs(col[c]);
        int p = c;
#pragma unroll
        for (int rr = c + 1; rr < 6; ++rr) {
            const double v = fabs(col[rr]);
            if (v > best) best = v, p = rr;
        }
        p = __builtin_amdgcn_readlane(p, c);   // lane c holds column c: its verdict is the pivot row
#pragma unroll
        for (int rr = c + 1; rr < 6; ++rr) {
            const double a = col[c], b = col[rr];
            col[c] = p == rr ? b : a;
            col[rr] = p == rr ? a : b;
        }
        const double d = cs_readlane_d(col[c], c);
        double f[6];
#pragma unroll
        for (int rr = 0; rr < 6; ++rr) f[rr] = cs_readlane_d(col[rr], c);
        const double q = col[c] / d;
        if (j > c) col[c] = q;
#pragma unroll
        for (int rr = 0; rr < 6; ++rr) {
            if (rr == c) continue;
            const double e = col[rr] - f[rr] * col[c];
            if (j > c) col[rr] = e;
        }
    }
#pragma unroll
    for (int rr = 0; rr < 6; ++rr) param[rr] = cs_readlane_d(col[rr], 6);
}

#endif  // __HIPCC__
