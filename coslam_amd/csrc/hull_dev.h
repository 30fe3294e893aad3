// hull_dev.h -- the convex hull of a point set in LDS by Quickhull rounds, one workgroup, every thread a share of the points (gfx950).
//
// The library's one definition of get2DConvexHull (a LibVisualSLAM function that is not in the reference tree).  Used by
// k_group_hull (grouping.hip: the hull's area) and k_merge_check (merge.hip: the hull's polygon as a mask).
//
// Every point outside the current polygon belongs to one edge, every edge takes its farthest point (LDS 64-bit max of the f64 distance's
// bits, lowest index among equals) and splits, points inside the new polygon drop out.  An edge is named by its start vertex and keeps its
// data in that point's slot, so the whole state is 32 bytes per point: xy 16, best distance 8, label 4, best index 4.  Each split adds the
// triangle (a, f, b) to the polygon: twice the area is the sum of the winners' cross products, summed per thread in round order.
#pragma once

#include "cs_common.h"

constexpr int HULL_POINT_BYTES = 32;   // xy 16, label 4, best distance 8, best index 4

// order-preserving 64-bit key of a double
__device__ __forceinline__ unsigned long long hull_key(double v) {
    const unsigned long long b = (unsigned long long)__double_as_longlong(v);
    return b >> 63 ? ~b : b | 0x8000000000000000ull;
}
// how far p lies OUTSIDE the edge a -> b of the hull polygon (> 0: outside; the polygon's interior is where every edge gives <= 0)
__device__ __forceinline__ double hull_out(double px, double py, double ax, double ay, double bx, double by) {
    return (px - ax) * (by - ay) - (py - ay) * (bx - ax);
}

// The hull of the n >= 3 points sXY[0 .. 2n) (x, y interleaved).  Called by all T threads of the workgroup (it holds barriers).
// Leaves in sLabel the vertex chain: a vertex's label is -2 - (index of the next vertex), every other point's is -1; with all x equal (a
// vertical line or one point) there is no vertex, a collinear set leaves the two-gon of its end points.  sBestD / sBestI are left cleared
// (0 / 0x7fffffff).  Returns THIS THREAD's share of twice the hull's area: the caller sums the shares (in a fixed order, for the same bits
// on every call).
template <int T>
__device__ __forceinline__ double hull_quick(double* sXY, unsigned long long* sBestD, int* sLabel, int* sBestI, int n) {
    __shared__ int sA, sB;
    __shared__ unsigned long long sKey[2];
    const int tid = threadIdx.x;
    double acc = 0.0;
    if (tid == 0) sKey[0] = ~0ull, sKey[1] = 0ull, sA = 0x7fffffff, sB = 0x7fffffff;
    __syncthreads();
    // a first two-gon: a point of least x and a point of greatest x (lowest index among equals); both lie on the hull's boundary
    for (int k = tid; k < n; k += T) {
        const unsigned long long key = hull_key(sXY[2 * k]);
        atomicMin(&sKey[0], key), atomicMax(&sKey[1], key);
        sBestD[k] = 0ull, sBestI[k] = 0x7fffffff;
    }
    __syncthreads();
    for (int k = tid; k < n; k += T) {
        const unsigned long long key = hull_key(sXY[2 * k]);
        if (key == sKey[0]) atomicMin(&sA, k);
        if (key == sKey[1]) atomicMin(&sB, k);
    }
    __syncthreads();
    const int a0 = sA, b0 = sB;
    int alive = 0;
    if (sKey[0] != sKey[1]) {
        const double ax = sXY[2 * a0], ay = sXY[2 * a0 + 1], bx = sXY[2 * b0], by = sXY[2 * b0 + 1];
        for (int k = tid; k < n; k += T) {
            const double px = sXY[2 * k], py = sXY[2 * k + 1];
            int lab = -1;
            if (k == a0) lab = -2 - b0;
            else if (k == b0) lab = -2 - a0;
            else if (hull_out(px, py, ax, ay, bx, by) > 0) lab = a0;
            else if (hull_out(px, py, bx, by, ax, ay) > 0) lab = b0;
            sLabel[k] = lab;
            alive |= lab >= 0;
        }
    } else {   // (all x equal: a vertical line or one point, area 0, no vertex)
        for (int k = tid; k < n; k += T) sLabel[k] = -1;
    }
    alive = __syncthreads_or(alive);
    while (alive) {   // one Quickhull round; every edge with a point outside it splits, so a round retires at least one point per edge
        for (int k = tid; k < n; k += T) {
            const int e = sLabel[k];
            if (e < 0) continue;
            const int b = -2 - sLabel[e];
            const double d = hull_out(sXY[2 * k], sXY[2 * k + 1], sXY[2 * e], sXY[2 * e + 1], sXY[2 * b], sXY[2 * b + 1]);
            atomicMax(&sBestD[e], (unsigned long long)__double_as_longlong(d));   // (d > 0: its bits order as the values do)
        }
        __syncthreads();
        for (int k = tid; k < n; k += T) {
            const int e = sLabel[k];
            if (e < 0) continue;
            const int b = -2 - sLabel[e];
            const double d = hull_out(sXY[2 * k], sXY[2 * k + 1], sXY[2 * e], sXY[2 * e + 1], sXY[2 * b], sXY[2 * b + 1]);
            if ((unsigned long long)__double_as_longlong(d) == sBestD[e]) atomicMin(&sBestI[e], k);
        }
        __syncthreads();
        // the alive points' new labels: only their own slots are written, only vertices' slots are read
        alive = 0;
        for (int k = tid; k < n; k += T) {
            const int e = sLabel[k];
            if (e < 0) continue;
            const int b = -2 - sLabel[e], f = sBestI[e];
            const double px = sXY[2 * k], py = sXY[2 * k + 1], ax = sXY[2 * e], ay = sXY[2 * e + 1], bx = sXY[2 * b], by = sXY[2 * b + 1];
            const double fx = sXY[2 * f], fy = sXY[2 * f + 1];
            int lab = -1;
            if (k == f) {
                lab = -2 - b;                                   // the edge f -> b
                acc += hull_out(px, py, ax, ay, bx, by);        // twice the triangle (a, f, b) that the polygon gains
            } else if (hull_out(px, py, ax, ay, fx, fy) > 0) lab = e;   // outside a -> f
            else if (hull_out(px, py, fx, fy, bx, by) > 0) lab = f;     // outside f -> b
            sLabel[k] = lab;
            alive |= lab >= 0;
        }
        alive = __syncthreads_or(alive);
        // the split edges' start vertices point at their winners; every vertex's round state is cleared
        for (int k = tid; k < n; k += T) {
            if (sLabel[k] > -2) continue;
            if (sBestI[k] != 0x7fffffff) sLabel[k] = -2 - sBestI[k];
            sBestD[k] = 0ull, sBestI[k] = 0x7fffffff;
        }
        __syncthreads();
    }
    return acc;
}
