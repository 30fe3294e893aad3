// posegraph.hip -- pose-graph relaxation of the non-key frames after a bundle adjustment, all camera graphs in one launch,
// gfx950.
//
// Replaces GlobalPoseGraph::computeNewCameraRotations (src/slam/SL_GlobalPoseEstimation.cpp:52-219) followed by
// computeNewCameraTranslations (:220-359) as RobustBundleRTS::updateNonKeyCameraPoses runs them for every camera after a BA
// (src/app/SL_CoSLAMRobustBA.cpp:230-247), plus the two loops around them that are pure data movement: the edges'
// relative transforms (constructCameraGraphs, :216-227, getRigidTransFromTo) and the copy of the adjusted key poses into
// the fixed nodes (output(), :283-294).
//
// What the reference solves: every edge (i -> j, R_ij, T_ij) with a free end gives the linear equations
//       R_j - R_ij R_i = 0   (9 per edge)        T_j - R_ij T_i = T_ij   (3 per edge)
// in the poses of the free nodes (fixed nodes go to the right-hand side), solved in the least-squares sense by a sparse QR
// (sparseSolveLin, un-vendored LibVisualSLAM), the 3x3 blocks of the first solution then replaced by the nearest rotation
// (approxRotationMat).  Two facts shape the kernel:
//   * the rotation system is the translation system three times over: column a of R_j obeys r_j - R_ij r_i = 0, so both
//     have the SAME 3-unknowns-per-node matrix A and only differ in the right-hand side.  One factorisation, 4 right-hand
//     sides (3 rotation columns + the translation), instead of a 9n and a 3n system;
//   * fixed nodes cut the graph: the free nodes fall into connected components that share nothing (for CoSLAM's chains:
//     the runs of non-key frames between two key frames).  Each component is an independent banded problem.
// So: one wave per component, normal equations N = A^T A (3x3 blocks: +I / R^T R on the diagonal per incident edge, -R_ij
// for a free-free edge) assembled lane-per-node in edge order (deterministic, no atomics) into LDS band storage, a band
// L D L^T (no square roots; the window update and the forward substitution of the 4 right-hand sides are one set of lane
// items, ONE barrier per unknown), back substitution with the band striped over a quad and folded on the DPP path, and
// a lane-per-node polar projection (Newton iteration X <- (X + X^-T) / 2: the orthogonal polar factor IS U V^T).  Band
// width follows from the component's node order (node index order: half-bandwidth 5 for a chain), so any topology the
// reference's API can express is solved -- a wide band only costs time.  Components too large for LDS run the same code
// out of an HBM workspace.  The least-squares solution is unique (full column rank), so QR on A and L D L^T of A^T A
// agree to rounding: cond(A^T A) ~ (chain length)^2, far from 1e16.  Tolerance stated in tests/test_posegraph_gpu.py.
//
//
// Edges with uncertainScale (src/app/SL_MergeCameraGroup.cpp:1025-1028 creates them; computeNewCameraTranslations4, :361-525,
// solves them) are the second half of this file (k_posegraph_relax_scaled): the translation system gains one
// column per scale id, [N B; B^T C] with the SAME node matrix N.  N is factored once with 4 + nS right-hand sides (3
// rotation columns, the translation, B's columns), the nS x nS Schur system is solved in one lane and the translation
// corrected.  The plan merges the components a scale ties together and moves the ends of the scaled edges ("border
// nodes") behind the interior, so that the interior keeps its narrow band and only the border block is dense; such a
// component runs on one whole workgroup, no atomics, fixed summation order.  Handles without a scaled edge, and the plain
// components of a scaled handle, run k_posegraph_relax exactly as before.
// Not built: a one-wave natural-order path for scaled components, and the workgroup path for plain components that are wide.
#include "cs_common.h"
#include "posegraph_view.h"

#include <algorithm>
#include <new>
#include <vector>

namespace {

constexpr int PG_LDS_DOUBLES = 7680;  // 60 KB: a component whose band + right-hand sides fit runs out of LDS

struct PgPlan {
    int nComp, nNodes, nEdges;
    const int* compPtr;         // nComp + 1, into compNode
    const int* compNode;        // global node index of every free node, component by component, ascending inside
    const int* compW;           // scalar half-bandwidth of the component's normal matrix
    const long long* compOff;   // < 0: LDS; else offset (doubles) of the component's workspace in `scratch`
    const int* adjPtr;          // per free-node slot, into adjEnt
    const int4* adjEnt;         // {edge, role (0: the node is id2, 1: it is id1), other end: position in the component or
                                //  -1 - global node when that end is fixed, 0}
    const int* nodeSlot;        // global node -> slot, -1 = fixed
    const int* ge1;             // global node index of the edges' ends
    const int* ge2;
    double* scratch;
    int* status;                // per component: 0 ok, 1 pivot <= 0 (a free node no edge constrains), 2 singular 3x3 block
};

// nearest orthogonal matrix of M (row-major): Newton iteration on the polar factor
__device__ __forceinline__ bool polar_rotation(const double M[9], double Q[9]) {
    double X[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) X[i] = M[i];
    bool ok = true;
    for (int it = 0; it < 12; ++it) {
        double C[9];  // cofactors: X^-T = C / det
        C[0] = X[4] * X[8] - X[5] * X[7];
        C[1] = X[5] * X[6] - X[3] * X[8];
        C[2] = X[3] * X[7] - X[4] * X[6];
        C[3] = X[2] * X[7] - X[1] * X[8];
        C[4] = X[0] * X[8] - X[2] * X[6];
        C[5] = X[1] * X[6] - X[0] * X[7];
        C[6] = X[1] * X[5] - X[2] * X[4];
        C[7] = X[2] * X[3] - X[0] * X[5];
        C[8] = X[0] * X[4] - X[1] * X[3];
        const double det = X[0] * C[0] + X[1] * C[1] + X[2] * C[2];
        if (!(fabs(det) > 1e-30)) {
            ok = false;
            break;
        }
        const double id = 0.5 / det;
        double delta = 0;
#pragma unroll
        for (int i = 0; i < 9; ++i) {
            const double y = 0.5 * X[i] + id * C[i];
            delta = fmax(delta, fabs(y - X[i]));
            X[i] = y;
        }
        if (delta < 1e-15) break;
    }
#pragma unroll
    for (int i = 0; i < 9; ++i) Q[i] = X[i];
    return ok;
}

// 1 / d for the pivots: hardware estimate + two Newton steps (the IEEE division sequence is three times as long and sits on
// the one dependency chain this kernel has)
__device__ __forceinline__ double pg_rcp(double d) {
    double r = __builtin_amdgcn_rcp(d);
    r = fma(fma(-d, r, 1.0), r, r);
    r = fma(fma(-d, r, 1.0), r, r);
    return r;
}

// lower-triangle pair (a, b), 1 <= b <= a, from its running index t = (a - 1) a / 2 + (b - 1)
__device__ __forceinline__ void pair_of(int t, int& a, int& b) {
    int r = (int)((sqrt(8.0 * t + 1.0) - 1.0) * 0.5);
    while ((r + 1) * (r + 2) / 2 <= t) ++r;
    while (r * (r + 1) / 2 > t) --r;
    a = r + 1;
    b = t - r * (r + 1) / 2 + 1;
}

// one component, one wave.  `Bnd` is LDS or the HBM workspace (two inlined copies, so the LDS one gets ds_ instructions):
//   Bnd[c * ld + a] = N[c + a][c], a = 0..w   the lower band, column by column
//   G[row * 4 + rhs]                          the 4 right-hand sides, then the solution
//   invd[c]                                   1 / pivot
__device__ __forceinline__ void pg_component(const PgPlan& p, int k, int lane, double* Bnd, const double* __restrict__ nodeR,
                                             const double* __restrict__ nodeT, const double* __restrict__ edgeR,
                                             const double* __restrict__ edgeT, double* __restrict__ newR,
                                             double* __restrict__ newT) {
    const int s0 = p.compPtr[k], cnt = p.compPtr[k + 1] - s0, n = 3 * cnt, w = p.compW[k], ld = w + 1;
    double* G = Bnd + (size_t)n * ld;
    double* invd = G + (size_t)n * 4;
    for (int i = lane; i < n * (ld + 5); i += 64) Bnd[i] = 0.0;
    __syncthreads();

    // ---- normal equations, one lane per free node, its edges in edge order ----
    for (int q = lane; q < cnt; q += 64) {
        const int slot = s0 + q;
        double D[9], g[12];
#pragma unroll
        for (int i = 0; i < 9; ++i) D[i] = 0.0;
#pragma unroll
        for (int i = 0; i < 12; ++i) g[i] = 0.0;
        for (int e = p.adjPtr[slot]; e < p.adjPtr[slot + 1]; ++e) {
            const int4 ent = p.adjEnt[e];
            double Re[9], b[12];  // b[i * 4 + rhs]: the edge's right-hand side
#pragma unroll
            for (int i = 0; i < 9; ++i) Re[i] = edgeR[9 * (size_t)ent.x + i];
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                b[4 * i] = b[4 * i + 1] = b[4 * i + 2] = 0.0;
                b[4 * i + 3] = edgeT[3 * (size_t)ent.x + i];
            }
            if (ent.y == 0) {  // this node is the edge's id2:  x_j - R x_i = b
                if (ent.z < 0) {  // id1 fixed: + R X_1 (:148-150, :330)
                    const size_t f = (size_t)(-1 - ent.z);
                    double X1[12];
#pragma unroll
                    for (int i = 0; i < 3; ++i) {
                        X1[4 * i] = nodeR[9 * f + 3 * i], X1[4 * i + 1] = nodeR[9 * f + 3 * i + 1];
                        X1[4 * i + 2] = nodeR[9 * f + 3 * i + 2], X1[4 * i + 3] = nodeT[3 * f + i];
                    }
#pragma unroll
                    for (int i = 0; i < 3; ++i)
#pragma unroll
                        for (int r = 0; r < 4; ++r)
                            b[4 * i + r] += (Re[3 * i] * X1[r] + Re[3 * i + 1] * X1[4 + r]) + Re[3 * i + 2] * X1[8 + r];
                }
                D[0] += 1.0, D[4] += 1.0, D[8] += 1.0;
#pragma unroll
                for (int i = 0; i < 12; ++i) g[i] += b[i];
                if (ent.z >= 0 && ent.z < q) {  // block (rows q, columns ent.z) = I^T (-R) = -R
#pragma unroll
                    for (int r = 0; r < 3; ++r)
#pragma unroll
                        for (int c = 0; c < 3; ++c) Bnd[(size_t)(3 * ent.z + c) * ld + (3 * (q - ent.z) + r - c)] -= Re[3 * r + c];
                }
            } else {  // this node is the edge's id1
                if (ent.z < 0) {  // id2 fixed: - X_2 (:183-193, :313-315)
                    const size_t f = (size_t)(-1 - ent.z);
#pragma unroll
                    for (int i = 0; i < 3; ++i) {
                        b[4 * i] -= nodeR[9 * f + 3 * i], b[4 * i + 1] -= nodeR[9 * f + 3 * i + 1];
                        b[4 * i + 2] -= nodeR[9 * f + 3 * i + 2], b[4 * i + 3] -= nodeT[3 * f + i];
                    }
                }
#pragma unroll
                for (int r = 0; r < 3; ++r)
#pragma unroll
                    for (int c = 0; c < 3; ++c) D[3 * r + c] += (Re[r] * Re[c] + Re[3 + r] * Re[3 + c]) + Re[6 + r] * Re[6 + c];
#pragma unroll
                for (int i = 0; i < 3; ++i)
#pragma unroll
                    for (int r = 0; r < 4; ++r) g[4 * i + r] -= (Re[i] * b[r] + Re[3 + i] * b[4 + r]) + Re[6 + i] * b[8 + r];
                if (ent.z >= 0 && ent.z < q) {  // block (rows q, columns ent.z) = (-R)^T I = -R^T
#pragma unroll
                    for (int r = 0; r < 3; ++r)
#pragma unroll
                        for (int c = 0; c < 3; ++c) Bnd[(size_t)(3 * ent.z + c) * ld + (3 * (q - ent.z) + r - c)] -= Re[3 * c + r];
                }
            }
        }
#pragma unroll
        for (int c = 0; c < 3; ++c)
#pragma unroll
            for (int r = c; r < 3; ++r)
                if (r - c <= w) Bnd[(size_t)(3 * q + c) * ld + (r - c)] += D[3 * r + c];
#pragma unroll
        for (int i = 0; i < 12; ++i) G[(size_t)(3 * q) * 4 + i] = g[i];
    }
    __syncthreads();

    // ---- band L D L^T (no square roots, columns stay unscaled: L = column / pivot), the forward substitution of the 4
    //      right-hand sides fused into the elimination step; one barrier per unknown ----
    const int nPairs = w * (w + 1) / 2, nItems = nPairs + 4 * w;
    bool bad = false;
    if (nItems <= 64) {  // chains (w = 5: 15 + 20 items) and other narrow bands: one item per lane, offsets fixed for the run
        int ia = 1, ib = 1, wo = 0;
        const bool isPair = lane < nPairs, isRhs = !isPair && lane < nItems;
        if (isPair) {
            pair_of(lane, ia, ib);
            wo = ib * ld + (ia - ib);  // N[j + a][j + b], relative to column j
        } else if (isRhs) {
            ia = 1 + ((lane - nPairs) >> 2);
            ib = (lane - nPairs) & 3;  // the right-hand side
            wo = 4 * ia + ib;          // G[j + a][rhs], relative to row j
        }
        double* col = Bnd;
        double* gj = G;
        for (int j = 0; j < n; ++j, col += ld, gj += 4) {
            const double d = col[0];
            if (!(d > 0.0)) bad = true;
            const double inv = pg_rcp(d > 0.0 ? d : 1.0);
            if (lane == 63) invd[j] = inv;
            if (j + ia < n) {
                if (isPair)
                    col[wo] -= (col[ia] * inv) * col[ib];
                else if (isRhs)
                    gj[wo] -= (col[ia] * inv) * gj[ib];
            }
            __syncthreads();
        }
    } else {
        for (int j = 0; j < n; ++j) {
            const int len = min(w, n - 1 - j);
            double* col = Bnd + (size_t)j * ld;
            const double d = col[0];
            if (!(d > 0.0)) bad = true;
            const double inv = pg_rcp(d > 0.0 ? d : 1.0);
            if (lane == 63) invd[j] = inv;
            for (int t = lane; t < nItems; t += 64) {
                if (t < nPairs) {
                    int a, b;
                    pair_of(t, a, b);
                    if (a <= len) col[b * ld + (a - b)] -= (col[a] * inv) * col[b];
                } else {
                    const int a = 1 + ((t - nPairs) >> 2), r = (t - nPairs) & 3;
                    if (a <= len) G[(size_t)(j + a) * 4 + r] -= (col[a] * inv) * G[(size_t)j * 4 + r];
                }
            }
            __syncthreads();
        }
    }
    // ---- back substitution x_j = (z_j - sum_a column_j[a] x_{j+a}) / pivot_j: lane = 4 * rhs + stripe of the band, the 4
    //      stripes of a quad folded on the DPP path ----
    {
        const int r = (lane >> 2) & 3, u = lane & 3;
        const double* col = Bnd + (size_t)(n - 1) * ld;
        double* gj = G + (size_t)(n - 1) * 4 + r;
        for (int j = n - 1; j >= 0; --j, col -= ld, gj -= 4) {
            const int len = min(w, n - 1 - j);
            double sum = 0.0;
            if (lane < 16)
                for (int a = 1 + u; a <= len; a += 4) sum += col[a] * gj[4 * a];
            sum += cs_dpp_d<0xB1, 0xf>(sum);  // quad_perm [1,0,3,2]
            sum += cs_dpp_d<0x4E, 0xf>(sum);  // quad_perm [2,3,0,1]
            if (lane < 16 && u == 0) gj[0] = (gj[0] - sum) * invd[j];
            __syncthreads();
        }
    }
    // ---- results: rotation = nearest orthogonal matrix of the 3 solved columns (:205-212), translation as solved (:346) ----
    bool singular = false;
    for (int q = lane; q < cnt; q += 64) {
        const size_t node = (size_t)p.compNode[s0 + q];
        double M[9], Q[9];
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int a = 0; a < 3; ++a) M[3 * i + a] = G[(size_t)(3 * q + i) * 4 + a];
        if (!polar_rotation(M, Q)) singular = true;
#pragma unroll
        for (int i = 0; i < 9; ++i) newR[9 * node + i] = Q[i];
#pragma unroll
        for (int i = 0; i < 3; ++i) newT[3 * node + i] = G[(size_t)(3 * q + i) * 4 + 3];
    }
    const int st = bad ? 1 : (__any(singular) ? 2 : 0);
    if (lane == 0) p.status[k] = st;
}

__global__ __launch_bounds__(64) void k_posegraph_relax(PgPlan p, const double* __restrict__ nodeR,
                                                        const double* __restrict__ nodeT, const double* __restrict__ edgeR,
                                                        const double* __restrict__ edgeT, double* __restrict__ newR,
                                                        double* __restrict__ newT) {
    extern __shared__ double pg_lds[];
    const int k = blockIdx.x, lane = threadIdx.x;
    if (k >= p.nComp) {  // the tail of the grid copies the fixed nodes (:213-214, :343-344)
        const int i = (k - p.nComp) * 64 + lane;
        if (i < p.nNodes && p.nodeSlot[i] < 0) {
#pragma unroll
            for (int q = 0; q < 9; ++q) newR[9 * (size_t)i + q] = nodeR[9 * (size_t)i + q];
#pragma unroll
            for (int q = 0; q < 3; ++q) newT[3 * (size_t)i + q] = nodeT[3 * (size_t)i + q];
        }
        return;
    }
    if (p.compOff[k] < 0)
        pg_component(p, k, lane, pg_lds, nodeR, nodeT, edgeR, edgeT, newR, newT);
    else
        pg_component(p, k, lane, p.scratch + p.compOff[k], nodeR, nodeT, edgeR, edgeT, newR, newT);
}

// relative transform of every edge from the poses of its ends (getRigidTransFromTo: R = R2 R1^T, t = t2 - R t1)
__global__ void k_posegraph_edges(int nEdges, const int* __restrict__ ge1, const int* __restrict__ ge2,
                                  const double* __restrict__ nodeR, const double* __restrict__ nodeT,
                                  double* __restrict__ edgeR, double* __restrict__ edgeT) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= nEdges || ge1[e] < 0) return;  // < 0: an uncertain-scale edge, its transform is given
    const size_t i = (size_t)ge1[e], j = (size_t)ge2[e];
    double R1[9], R2[9], R[9];
#pragma unroll
    for (int q = 0; q < 9; ++q) R1[q] = nodeR[9 * i + q], R2[q] = nodeR[9 * j + q];
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) R[3 * r + c] = (R2[3 * r] * R1[3 * c] + R2[3 * r + 1] * R1[3 * c + 1]) + R2[3 * r + 2] * R1[3 * c + 2];
#pragma unroll
    for (int q = 0; q < 9; ++q) edgeR[9 * (size_t)e + q] = R[q];
#pragma unroll
    for (int r = 0; r < 3; ++r)
        edgeT[3 * (size_t)e + r] = nodeT[3 * j + r] - ((R[3 * r] * nodeT[3 * i] + R[3 * r + 1] * nodeT[3 * i + 1]) + R[3 * r + 2] * nodeT[3 * i + 2]);
}

__global__ void k_posegraph_set_poses(int n, const int* __restrict__ nodeIdx, const double* __restrict__ R,
                                      const double* __restrict__ t, double* __restrict__ nodeR, double* __restrict__ nodeT) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int node = nodeIdx[i];
    if (node < 0) return;
#pragma unroll
    for (int q = 0; q < 9; ++q) nodeR[9 * (size_t)node + q] = R[9 * (size_t)i + q];
#pragma unroll
    for (int q = 0; q < 3; ++q) nodeT[3 * (size_t)node + q] = t[3 * (size_t)i + q];
}


// ---------------------------------------------------------------------------------------------------------------------
// components with uncertain-scale edges (computeNewCameraTranslations4): one workgroup per component
// ---------------------------------------------------------------------------------------------------------------------
constexpr int PGS_THREADS = 256;   // 4 waves
constexpr int PGS_WAVES = PGS_THREADS / 64;
constexpr int PGS_MAX_SCALES = 4;  // scale unknowns per component (the reference only ever uses id 0)
constexpr int PGS_MAX_RHS = 4 + PGS_MAX_SCALES;
// the scale solve's small LDS block: Schur matrix | right-hand side | C's diagonal | the scales | failed
constexpr int PGS_SH_S = 0, PGS_SH_H = PGS_SH_S + PGS_MAX_SCALES * PGS_MAX_SCALES, PGS_SH_C = PGS_SH_H + PGS_MAX_SCALES,
              PGS_SH_X = PGS_SH_C + PGS_MAX_SCALES, PGS_SH_FAIL = PGS_SH_X + PGS_MAX_SCALES, PGS_SH_DOUBLES = PGS_SH_FAIL + 1;

struct PgsPlan {
    int nComp;
    const int* compPtr;        // nComp + 1, into compNode
    const int* compNode;       // global node index: the component's interior nodes ascending, then its border nodes ascending
    const int4* compDim;       // {interior nodes, border nodes, scalar half-bandwidth of the interior, scales}
    const long long* compOff;  // < 0: LDS; else offset (doubles) of the component's workspace in `scratch`
    const int* adjPtr;         // per node slot, into adjEnt
    const int4* adjEnt;        // {edge, role, other end (position or -1 - global node), scale of the edge in the component or -1}
    const int* sePtr;          // nComp + 1, into seEnt
    const int4* seEnt;         // the scaled edges in edge order: {edge, id1's position or -1 - global, id2's, scale}
    double* scratch;
    int* status;               // per component: as PgPlan::status, 3 = a scale unknown is not determined
};

// Workspace W of a component (n_I = 3 * interior, n_B = 3 * border, nr = 4 + scales, nT = n_B + nr "trailing rows"):
//   Bnd[c * ld + a]   = N[c + a][c]                     the interior's lower band, column by column (ld = w + 1)
//   Tr[c * nT + r]    = N[n_I + r][c]        r <  n_B   the border rows over the interior columns (dense: they fill in)
//                     = right-hand side r - n_B, row c   r >= n_B   (a right-hand side is eliminated like a matrix row)
//   Dd[r * nT + c]    = N[n_I + r][n_I + c]  c <= r < n_B  the border block, lower triangle
//                     = right-hand side r - n_B, row n_I + c        r >= n_B
//   invd[c]           = 1 / pivot
// After the solve the right-hand-side slots hold the solution.
__device__ __forceinline__ void pgs_component(const PgsPlan& p, int k, int tid, double* W, double* sh, const double* __restrict__ nodeR,
                                              const double* __restrict__ nodeT, const double* __restrict__ edgeR,
                                              const double* __restrict__ edgeT, double* __restrict__ newR,
                                              double* __restrict__ newT, double* __restrict__ edgeS) {
    const int4 dim = p.compDim[k];
    const int s0 = p.compPtr[k], ni = dim.x, nb = dim.y, w = dim.z, nS = dim.w;
    const int cnt = ni + nb, nI = 3 * ni, nB = 3 * nb, nr = 4 + nS, nT = nB + nr, ld = w + 1, n = nI + nB;
    const int wave = tid >> 6, lane = tid & 63;
    double* Bnd = W;
    double* Tr = Bnd + (size_t)nI * ld;
    double* Dd = Tr + (size_t)nI * nT;
    double* invd = Dd + (size_t)nT * nT;
    const size_t tot = (size_t)nI * (ld + nT) + (size_t)nT * nT + n;
    for (size_t i = tid; i < tot; i += PGS_THREADS) W[i] = 0.0;
    __syncthreads();

    // ---- normal equations, one lane per free node, its edges in edge order.  Row of an edge (i -> j, R, t):
    //      x_j - R x_i = b, b = 0 for the rotation columns, t for the translation of a plain edge, 0 for the translation of
    //      a scaled edge (:450-456: its t goes into the scale's column as -t), plus what a fixed end gives (:476-478, :495)
    for (int q = tid; q < cnt; q += PGS_THREADS) {
        const int slot = s0 + q;
        double D[9], g[3 * PGS_MAX_RHS];
#pragma unroll
        for (int i = 0; i < 9; ++i) D[i] = 0.0;
#pragma unroll
        for (int i = 0; i < 3 * PGS_MAX_RHS; ++i) g[i] = 0.0;
        for (int e = p.adjPtr[slot]; e < p.adjPtr[slot + 1]; ++e) {
            const int4 ent = p.adjEnt[e];
            double Re[9], b[3 * PGS_MAX_RHS];  // b[i * PGS_MAX_RHS + rhs]
#pragma unroll
            for (int i = 0; i < 9; ++i) Re[i] = edgeR[9 * (size_t)ent.x + i];
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                const double te = edgeT[3 * (size_t)ent.x + i];
#pragma unroll
                for (int r = 0; r < PGS_MAX_RHS; ++r) b[PGS_MAX_RHS * i + r] = 0.0;
                if (ent.w < 0) b[PGS_MAX_RHS * i + 3] = te;
#pragma unroll
                for (int r = 0; r < PGS_MAX_SCALES; ++r)
                    if (ent.w == r) b[PGS_MAX_RHS * i + 4 + r] = -te;
            }
            const int z = ent.z;
            if (ent.y == 0) {  // this node is the edge's id2
                if (z < 0) {   // id1 fixed: + R X_1
                    const size_t f = (size_t)(-1 - z);
                    double X1[12];
#pragma unroll
                    for (int i = 0; i < 3; ++i) {
                        X1[4 * i] = nodeR[9 * f + 3 * i], X1[4 * i + 1] = nodeR[9 * f + 3 * i + 1];
                        X1[4 * i + 2] = nodeR[9 * f + 3 * i + 2], X1[4 * i + 3] = nodeT[3 * f + i];
                    }
#pragma unroll
                    for (int i = 0; i < 3; ++i)
#pragma unroll
                        for (int r = 0; r < 4; ++r)
                            b[PGS_MAX_RHS * i + r] += (Re[3 * i] * X1[r] + Re[3 * i + 1] * X1[4 + r]) + Re[3 * i + 2] * X1[8 + r];
                }
                D[0] += 1.0, D[4] += 1.0, D[8] += 1.0;
#pragma unroll
                for (int i = 0; i < 3 * PGS_MAX_RHS; ++i) g[i] += b[i];
            } else {  // this node is the edge's id1
                if (z < 0) {  // id2 fixed: - X_2
                    const size_t f = (size_t)(-1 - z);
#pragma unroll
                    for (int i = 0; i < 3; ++i) {
                        b[PGS_MAX_RHS * i] -= nodeR[9 * f + 3 * i], b[PGS_MAX_RHS * i + 1] -= nodeR[9 * f + 3 * i + 1];
                        b[PGS_MAX_RHS * i + 2] -= nodeR[9 * f + 3 * i + 2], b[PGS_MAX_RHS * i + 3] -= nodeT[3 * f + i];
                    }
                }
#pragma unroll
                for (int r = 0; r < 3; ++r)
#pragma unroll
                    for (int c = 0; c < 3; ++c) D[3 * r + c] += (Re[r] * Re[c] + Re[3 + r] * Re[3 + c]) + Re[6 + r] * Re[6 + c];
#pragma unroll
                for (int i = 0; i < 3; ++i)
#pragma unroll
                    for (int r = 0; r < PGS_MAX_RHS; ++r)
                        g[PGS_MAX_RHS * i + r] -= (Re[i] * b[r] + Re[3 + i] * b[PGS_MAX_RHS + r]) + Re[6 + i] * b[2 * PGS_MAX_RHS + r];
            }
            if (z >= 0 && z < q) {  // block (rows q, columns z): -R when this node is id2, -R^T when it is id1
#pragma unroll
                for (int r = 0; r < 3; ++r)
#pragma unroll
                    for (int c = 0; c < 3; ++c) {
                        const double v = ent.y == 0 ? Re[3 * r + c] : Re[3 * c + r];
                        if (q < ni)
                            Bnd[(size_t)(3 * z + c) * ld + (3 * (q - z) + r - c)] -= v;
                        else if (z < ni)
                            Tr[(size_t)(3 * z + c) * nT + (3 * (q - ni) + r)] -= v;
                        else
                            Dd[(size_t)(3 * (q - ni) + r) * nT + (3 * (z - ni) + c)] -= v;
                    }
            }
        }
#pragma unroll
        for (int c = 0; c < 3; ++c)
#pragma unroll
            for (int r = c; r < 3; ++r) {
                if (q < ni)
                    Bnd[(size_t)(3 * q + c) * ld + (r - c)] += D[3 * r + c];
                else
                    Dd[(size_t)(3 * (q - ni) + r) * nT + (3 * (q - ni) + c)] += D[3 * r + c];
            }
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int r = 0; r < PGS_MAX_RHS; ++r) {  // (unrolled: g stays in registers)
                if (r >= nr) continue;
                if (q < ni)
                    Tr[(size_t)(3 * q + i) * nT + nB + r] = g[PGS_MAX_RHS * i + r];
                else
                    Dd[(size_t)(nB + r) * nT + (3 * (q - ni) + i)] = g[PGS_MAX_RHS * i + r];
            }
    }
    __syncthreads();

    // ---- L D L^T, columns unscaled (L = column / pivot).  An interior column updates its band window, the trailing rows
    //      over the window, and the trailing block; every item reads column j only and writes elsewhere: one barrier per
    //      unknown.  Items are dealt to the waves by row, to the lanes along the row: each sum has one owner and one order.
    bool bad = false;
    for (int j = 0; j < nI; ++j) {
        const int len = min(w, nI - 1 - j);
        double* col = Bnd + (size_t)j * ld;
        const double* trj = Tr + (size_t)j * nT;
        const double d = col[0];
        if (!(d > 0.0)) bad = true;
        const double inv = pg_rcp(d > 0.0 ? d : 1.0);
        if (tid == 0) invd[j] = inv;
        for (int b = 1 + wave; b <= len; b += PGS_WAVES) {
            const double cb = col[b] * inv;
            for (int a = b + lane; a <= len; a += 64) col[(size_t)b * ld + (a - b)] -= col[a] * cb;
        }
        for (int a = 1 + wave; a <= len; a += PGS_WAVES) {
            const double ca = col[a] * inv;
            for (int r = lane; r < nT; r += 64) {
                const double v = trj[r];
                if (v != 0.0) Tr[(size_t)(j + a) * nT + r] -= v * ca;
            }
        }
        for (int r = wave; r < nT; r += PGS_WAVES) {
            const double v = trj[r] * inv;
            if (v == 0.0) continue;
            const int cmax = min(r, nB - 1);
            for (int c = lane; c <= cmax; c += 64) Dd[(size_t)r * nT + c] -= v * trj[c];
        }
        __syncthreads();
    }
    for (int j = 0; j < nB; ++j) {  // the border block, dense
        const double d = Dd[(size_t)j * nT + j];
        if (!(d > 0.0)) bad = true;
        const double inv = pg_rcp(d > 0.0 ? d : 1.0);
        if (tid == 0) invd[nI + j] = inv;
        for (int r = j + 1 + wave; r < nT; r += PGS_WAVES) {
            const double v = Dd[(size_t)r * nT + j] * inv;
            if (v == 0.0) continue;
            const int cmax = min(r, nB - 1);
            for (int c = j + 1 + lane; c <= cmax; c += 64) Dd[(size_t)r * nT + c] -= v * Dd[(size_t)c * nT + j];
        }
        __syncthreads();
    }
    // ---- back substitution.  Border: one lane per right-hand side (it reads and writes its own row only) ----
    if (tid < nr) {
        double* x = Dd + (size_t)(nB + tid) * nT;
        for (int c = nB - 1; c >= 0; --c) {
            double sum = 0.0;
            for (int c2 = c + 1; c2 < nB; ++c2) sum += Dd[(size_t)c2 * nT + c] * x[c2];
            x[c] = (x[c] - sum) * invd[nI + c];
        }
    }
    __syncthreads();
    for (int t = tid; t < nI * nr; t += PGS_THREADS) {  // the border's part of every interior row
        const int j = t / nr, r = t - j * nr;
        const double* trj = Tr + (size_t)j * nT;
        const double* x = Dd + (size_t)(nB + r) * nT;
        double sum = 0.0;
        for (int c = 0; c < nB; ++c) sum += trj[c] * x[c];
        Tr[(size_t)j * nT + nB + r] -= sum;
    }
    __syncthreads();
    {  // interior: lane = 4 * rhs + stripe of the band, the 4 stripes of a quad folded on the DPP path
        const int r = tid >> 2, u = tid & 3;
        const bool act = r < nr;
        for (int j = nI - 1; j >= 0; --j) {
            const int len = min(w, nI - 1 - j);
            const double* col = Bnd + (size_t)j * ld;
            double* gj = Tr + (size_t)j * nT + nB + (act ? r : 0);
            double sum = 0.0;
            if (act)
                for (int a = 1 + u; a <= len; a += 4) sum += col[a] * gj[(size_t)a * nT];
            sum += cs_dpp_d<0xB1, 0xf>(sum);  // quad_perm [1,0,3,2]
            sum += cs_dpp_d<0x4E, 0xf>(sum);  // quad_perm [2,3,0,1]
            if (act && u == 0) gj[0] = (gj[0] - sum) * invd[j];
            __syncthreads();
        }
    }
    auto sol = [&](int pos, int i, int r) -> double {
        return pos < ni ? Tr[(size_t)(3 * pos + i) * nT + nB + r] : Dd[(size_t)(nB + r) * nT + (3 * (pos - ni) + i)];
    };
    // ---- the scales: with x0 = N^-1 g_t and Y = N^-1 B in hand, (C - B^T Y) s = h - B^T x0, written over the scaled edges'
    //      rows (B^T v = sum over the scale's edges of -t . (v_j - R v_i)); one lane, edge order ----
    if (tid == 0) {
        // (in LDS: the edges index them by their scale, registers would go to scratch)
        double *S = sh + PGS_SH_S, *h = sh + PGS_SH_H, *C = sh + PGS_SH_C, *sc = sh + PGS_SH_X;
        for (int a = 0; a < PGS_MAX_SCALES; ++a) {
            h[a] = C[a] = sc[a] = 0.0;
            for (int b = 0; b < PGS_MAX_SCALES; ++b) S[a * PGS_MAX_SCALES + b] = 0.0;
        }
        for (int e = p.sePtr[k]; e < p.sePtr[k + 1]; ++e) {
            const int4 ent = p.seEnt[e];
            if (ent.y < 0 && ent.z < 0) continue;  // fixed-fixed: no row (:368)
            double Re[9], te[3], rr[3];
            for (int i = 0; i < 9; ++i) Re[i] = edgeR[9 * (size_t)ent.x + i];
            for (int i = 0; i < 3; ++i) te[i] = edgeT[3 * (size_t)ent.x + i], rr[i] = 0.0;
            if (ent.y < 0) {
                const size_t f = (size_t)(-1 - ent.y);
                for (int i = 0; i < 3; ++i) rr[i] += (Re[3 * i] * nodeT[3 * f] + Re[3 * i + 1] * nodeT[3 * f + 1]) + Re[3 * i + 2] * nodeT[3 * f + 2];
            }
            if (ent.z < 0) {
                const size_t f = (size_t)(-1 - ent.z);
                for (int i = 0; i < 3; ++i) rr[i] -= nodeT[3 * f + i];
            }
            double tt = (te[0] * te[0] + te[1] * te[1]) + te[2] * te[2];
            C[ent.w] += tt;
            S[ent.w * PGS_MAX_SCALES + ent.w] += tt;
            for (int r = 3; r < nr; ++r) {  // (A v)_e for v = x0 and every Y column
                double v1[3] = {0, 0, 0}, av[3];
                if (ent.y >= 0)
                    for (int i = 0; i < 3; ++i) v1[i] = sol(ent.y, i, r);
                for (int i = 0; i < 3; ++i) {
                    av[i] = -((Re[3 * i] * v1[0] + Re[3 * i + 1] * v1[1]) + Re[3 * i + 2] * v1[2]);
                    if (ent.z >= 0) av[i] += sol(ent.z, i, r);
                }
                if (r == 3)
                    h[ent.w] -= (te[0] * (rr[0] - av[0]) + te[1] * (rr[1] - av[1])) + te[2] * (rr[2] - av[2]);
                else
                    S[ent.w * PGS_MAX_SCALES + (r - 4)] += (te[0] * av[0] + te[1] * av[1]) + te[2] * av[2];
            }
        }
        bool ok = true;  // Gaussian elimination of the small symmetric positive definite system, no pivoting
        for (int a = 0; a < nS; ++a) {
            const double piv = S[a * PGS_MAX_SCALES + a];
            if (!(piv > 1e-12 * C[a])) {
                ok = false;
                break;
            }
            for (int b = a + 1; b < nS; ++b) {
                const double f = S[b * PGS_MAX_SCALES + a] / piv;
                for (int c = a; c < nS; ++c) S[b * PGS_MAX_SCALES + c] -= f * S[a * PGS_MAX_SCALES + c];
                h[b] -= f * h[a];
            }
        }
        if (ok)
            for (int a = nS - 1; a >= 0; --a) {
                double v = h[a];
                for (int b = a + 1; b < nS; ++b) v -= S[a * PGS_MAX_SCALES + b] * sc[b];
                sc[a] = v / S[a * PGS_MAX_SCALES + a];
            }
        for (int a = 0; a < PGS_MAX_SCALES; ++a) sc[a] = ok ? sc[a] : 0.0;
        sh[PGS_SH_FAIL] = ok ? 0.0 : 1.0;
        for (int e = p.sePtr[k]; e < p.sePtr[k + 1]; ++e) {  // CamPoseEdge::s (:515-522), fixed-fixed edges included
            const int4 ent = p.seEnt[e];
            edgeS[ent.x] = ok ? sc[ent.w] : 0.0;
        }
    }
    __syncthreads();
    // ---- results: rotations as in k_posegraph_relax, translation x0 - Y s ----
    bool singular = false;
    for (int q = tid; q < cnt; q += PGS_THREADS) {
        const size_t node = (size_t)p.compNode[s0 + q];
        double M[9], Q[9];
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int a = 0; a < 3; ++a) M[3 * i + a] = sol(q, i, a);
        if (!polar_rotation(M, Q)) singular = true;
#pragma unroll
        for (int i = 0; i < 9; ++i) newR[9 * node + i] = Q[i];
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            double v = sol(q, i, 3);
            for (int a = 0; a < nS; ++a) v -= sol(q, i, 4 + a) * sh[PGS_SH_X + a];
            newT[3 * node + i] = v;
        }
    }
    const int anySing = __syncthreads_or(singular ? 1 : 0);
    const int st = bad ? 1 : (sh[PGS_SH_FAIL] != 0.0 ? 3 : (anySing ? 2 : 0));
    if (tid == 0) p.status[k] = st;
}

__global__ __launch_bounds__(PGS_THREADS) void k_posegraph_relax_scaled(PgsPlan p, const double* __restrict__ nodeR,
                                                                        const double* __restrict__ nodeT,
                                                                        const double* __restrict__ edgeR,
                                                                        const double* __restrict__ edgeT, double* __restrict__ newR,
                                                                        double* __restrict__ newT, double* __restrict__ edgeS) {
    extern __shared__ double pgs_lds[];
    __shared__ double sh[PGS_SH_DOUBLES];
    const int k = blockIdx.x, tid = threadIdx.x;
    if (k >= p.nComp) return;
    if (p.compOff[k] < 0)
        pgs_component(p, k, tid, pgs_lds, sh, nodeR, nodeT, edgeR, edgeT, newR, newT, edgeS);
    else
        pgs_component(p, k, tid, p.scratch + p.compOff[k], sh, nodeR, nodeT, edgeR, edgeT, newR, newT, edgeS);
}

int find_root(std::vector<int>& parent, int i) {
    while (parent[i] != i) {
        parent[i] = parent[parent[i]];
        i = parent[i];
    }
    return i;
}

}  // namespace

struct cs_posegraph {
    int device = 0;
    int nGraphs = 0, nNodes = 0, nEdges = 0, nComp = 0;
    size_t ldsBytes = 0;
    // components with uncertain-scale edges (cs_posegraph_create_scaled); status and compGraph hold them behind the plain ones
    int nSComp = 0, nScales = 0, nBorder = 0, maxInteriorW = 0;
    size_t sLdsBytes = 0;
    PgsPlan splan{};
    char* dev = nullptr;  // one allocation: plan arrays | status | workspace
    PgPlan plan{};
    std::vector<int> compGraph;  // component -> graph (error messages)
    double* dIn = nullptr;  // staging of the host form (inside `dev`)
};

static int pg_create(const char* fn, int device, int nGraphs, const int* nodePtr, const int* edgePtr, const unsigned char* fixed,
                     const int* id1, const int* id2, const int* scaleId, cs_posegraph** out) {
    if (!out) {
        cs_set_error("%s: null out pointer", fn);
        return CS_ERR_INVALID;
    }
    *out = nullptr;
    if (nGraphs < 0 || !nodePtr || !edgePtr || nodePtr[0] != 0 || edgePtr[0] != 0) {
        cs_set_error("%s: bad graph table", fn);
        return CS_ERR_INVALID;
    }
    for (int g = 0; g < nGraphs; ++g)
        if (nodePtr[g + 1] < nodePtr[g] || edgePtr[g + 1] < edgePtr[g]) {
            cs_set_error("%s: nodePtr / edgePtr must be non-decreasing (graph %d)", fn, g);
            return CS_ERR_INVALID;
        }
    const int N = nGraphs ? nodePtr[nGraphs] : 0, E = nGraphs ? edgePtr[nGraphs] : 0;
    if ((N > 0 && !fixed) || (E > 0 && (!id1 || !id2))) {
        cs_set_error("%s: null pointer", fn);
        return CS_ERR_INVALID;
    }
    // global ends of the edges, connected components of the free nodes (fixed nodes cut the graph)
    std::vector<int> ge1(E), ge2(E), parent(N);
    for (int i = 0; i < N; ++i) parent[i] = i;
    for (int g = 0; g < nGraphs; ++g) {
        const int nb = nodePtr[g], nn = nodePtr[g + 1] - nb;
        for (int e = edgePtr[g]; e < edgePtr[g + 1]; ++e) {
            if (id1[e] < 0 || id1[e] >= nn || id2[e] < 0 || id2[e] >= nn || id1[e] == id2[e]) {
                cs_set_error("%s: edge %d of graph %d joins nodes %d -> %d (graph has %d nodes)", fn, e - edgePtr[g], g, id1[e],
                             id2[e], nn);
                return CS_ERR_INVALID;
            }
            ge1[e] = nb + id1[e];
            ge2[e] = nb + id2[e];
            if (!fixed[ge1[e]] && !fixed[ge2[e]]) {
                const int a = find_root(parent, ge1[e]), b = find_root(parent, ge2[e]);
                if (a != b) parent[std::max(a, b)] = std::min(a, b);  // root = smallest node: components come out in node order
            }
        }
    }
    // uncertain-scale edges: a scale ties the components of its edges' free ends together; those components leave the plain plan
    std::vector<unsigned char> inScaled(N, 0);
    std::vector<int> scaleAnchor(E, -1);  // per edge slot edgePtr[g] + id: a free node of scale id of graph g
    bool anyScaled = false;
    if (scaleId) {
        for (int g = 0; g < nGraphs; ++g) {
            const int eb = edgePtr[g], ne = edgePtr[g + 1] - eb;
            for (int e = eb; e < eb + ne; ++e) {
                const int sid = scaleId[e];
                if (sid < 0) continue;
                if (sid >= ne) {
                    cs_set_error("%s: edge %d of graph %d has scale id %d, the graph has %d edges (ids must be below the edge count)", fn,
                                 e - eb, g, sid, ne);
                    return CS_ERR_INVALID;
                }
                anyScaled = true;
                for (int end = 0; end < 2; ++end) {
                    const int nd = end ? ge2[e] : ge1[e];
                    if (fixed[nd]) continue;
                    if (scaleAnchor[eb + sid] < 0) scaleAnchor[eb + sid] = nd;
                    const int a = find_root(parent, scaleAnchor[eb + sid]), b = find_root(parent, nd);
                    if (a != b) parent[std::max(a, b)] = std::min(a, b);
                }
            }
            for (int e = eb; e < eb + ne; ++e)
                if (scaleId[e] >= 0 && scaleAnchor[eb + scaleId[e]] < 0) {
                    cs_set_error("%s: scale id %d of graph %d is used by edges between fixed nodes only (a zero column)", fn, scaleId[e], g);
                    return CS_ERR_INVALID;
                }
        }
        if (anyScaled) {
            std::vector<unsigned char> rootScaled(N, 0);
            for (int e = 0; e < E; ++e)
                if (scaleId[e] >= 0) {
                    if (!fixed[ge1[e]]) rootScaled[find_root(parent, ge1[e])] = 1;
                    if (!fixed[ge2[e]]) rootScaled[find_root(parent, ge2[e])] = 1;
                }
            for (int i = 0; i < N; ++i)
                if (!fixed[i] && rootScaled[find_root(parent, i)]) inScaled[i] = 1;
        }
    }
    std::vector<int> compOfRoot(N, -1), nodeSlot(N, -1), nodePos(N, -1), compPtr(1, 0), compNode, compGraph;
    int nComp = 0;
    std::vector<int> graphOf(N);
    for (int g = 0; g < nGraphs; ++g)
        for (int i = nodePtr[g]; i < nodePtr[g + 1]; ++i) graphOf[i] = g;
    {
        std::vector<int> compCount;
        for (int i = 0; i < N; ++i) {
            if (fixed[i] || inScaled[i]) continue;
            const int r = find_root(parent, i);
            if (compOfRoot[r] < 0) {
                compOfRoot[r] = nComp++;
                compCount.push_back(0);
                compGraph.push_back(graphOf[i]);
            }
            ++compCount[compOfRoot[r]];
        }
        for (int c = 0; c < nComp; ++c) compPtr.push_back(compPtr.back() + compCount[c]);
        compNode.resize(compPtr.back());
        std::vector<int> fill(compPtr.begin(), compPtr.end() - 1);
        for (int i = 0; i < N; ++i) {
            if (fixed[i] || inScaled[i]) continue;
            const int c = compOfRoot[find_root(parent, i)];
            nodePos[i] = fill[c] - compPtr[c];
            nodeSlot[i] = fill[c];
            compNode[fill[c]++] = i;
        }
    }
    const int nFree = (int)compNode.size();
    // adjacency of the free nodes in edge order, block bandwidth of every component
    std::vector<int> adjPtr(nFree + 1, 0), compBw(nComp, 0);
    for (int e = 0; e < E; ++e) {
        const int s1 = nodeSlot[ge1[e]], s2 = nodeSlot[ge2[e]];
        if (s1 >= 0) ++adjPtr[s1 + 1];
        if (s2 >= 0) ++adjPtr[s2 + 1];
        if (s1 >= 0 && s2 >= 0) {
            const int c = compOfRoot[find_root(parent, ge1[e])];
            compBw[c] = std::max(compBw[c], std::abs(nodePos[ge1[e]] - nodePos[ge2[e]]));
        }
    }
    for (int s = 0; s < nFree; ++s) adjPtr[s + 1] += adjPtr[s];
    std::vector<int4> adjEnt(adjPtr[nFree]);
    {
        std::vector<int> fill(adjPtr.begin(), adjPtr.end() - 1);
        for (int e = 0; e < E; ++e) {
            const int s1 = nodeSlot[ge1[e]], s2 = nodeSlot[ge2[e]];
            if (s2 >= 0) adjEnt[fill[s2]++] = make_int4(e, 0, s1 >= 0 ? nodePos[ge1[e]] : -1 - ge1[e], 0);
            if (s1 >= 0) adjEnt[fill[s1]++] = make_int4(e, 1, s2 >= 0 ? nodePos[ge2[e]] : -1 - ge2[e], 0);
        }
    }
    std::vector<int> compW(nComp);
    std::vector<long long> compOff(nComp);
    size_t ldsDoubles = 0, scratchDoubles = 0;
    for (int c = 0; c < nComp; ++c) {
        const int n = 3 * (compPtr[c + 1] - compPtr[c]);
        compW[c] = std::min(3 * compBw[c] + 2, n - 1);
        const size_t need = (size_t)n * (compW[c] + 1 + 4 + 1);  // band | right-hand sides | 1 / pivots
        if (need <= (size_t)PG_LDS_DOUBLES) {
            compOff[c] = -1;
            ldsDoubles = std::max(ldsDoubles, need);
        } else {
            compOff[c] = (long long)scratchDoubles;
            scratchDoubles += need;
        }
    }
    // ---- the components with scaled edges: interior nodes in node order (frame-major for a merge graph: the band stays
    //      narrow), the ends of the scaled edges behind them as the dense border ----
    int nSComp = 0, nScalesTotal = 0, nBorderTotal = 0, maxInteriorW = 0;
    std::vector<int> sCompPtr(1, 0), sCompNode, sAdjPtr(1, 0), sePtr(1, 0), sCompGraph;
    std::vector<int4> sCompDim, sAdjEnt, seEnt;
    std::vector<long long> sCompOff;
    size_t sLdsDoubles = 0;
    if (anyScaled) {
        std::vector<int> sCompOf(N, -1), sPos(N, -1);
        std::vector<unsigned char> border(N, 0);
        for (int e = 0; e < E; ++e)
            if (scaleId[e] >= 0) border[ge1[e]] = border[ge2[e]] = 1;
        std::vector<std::vector<int>> members;
        for (int i = 0; i < N; ++i) {
            if (!inScaled[i]) continue;
            const int r = find_root(parent, i);
            if (sCompOf[r] < 0) {
                sCompOf[r] = nSComp++;
                members.emplace_back();
                sCompGraph.push_back(graphOf[i]);
            }
            members[sCompOf[r]].push_back(i);
        }
        auto compOfNode = [&](int nd) { return sCompOf[find_root(parent, nd)]; };
        std::vector<std::vector<int>> compScales(nSComp), compEdges(nSComp);
        for (int g = 0; g < nGraphs; ++g)
            for (int e = edgePtr[g]; e < edgePtr[g + 1]; ++e) {
                const int f1 = !fixed[ge1[e]] && inScaled[ge1[e]], f2 = !fixed[ge2[e]] && inScaled[ge2[e]];
                int c = f1 ? compOfNode(ge1[e]) : (f2 ? compOfNode(ge2[e]) : -1);
                if (scaleId[e] >= 0) {
                    c = compOfNode(scaleAnchor[edgePtr[g] + scaleId[e]]);
                    compScales[c].push_back(scaleId[e]);
                }
                if (c >= 0) compEdges[c].push_back(e);
            }
        for (int c = 0; c < nSComp; ++c) {
            std::vector<int>& sc = compScales[c];
            std::sort(sc.begin(), sc.end());
            sc.erase(std::unique(sc.begin(), sc.end()), sc.end());  // ascending by id: the reference's column order (:397-403)
            if ((int)sc.size() > PGS_MAX_SCALES) {
                cs_set_error("%s: a component of graph %d has %d scale unknowns, at most %d are supported", fn, sCompGraph[c], (int)sc.size(),
                             PGS_MAX_SCALES);
                return CS_ERR_INVALID;
            }
            int ni = 0, nb = 0;
            for (int nd : members[c])
                if (!border[nd]) sPos[nd] = ni++, sCompNode.push_back(nd);
            for (int nd : members[c])
                if (border[nd]) sPos[nd] = ni + nb++, sCompNode.push_back(nd);
            sCompPtr.push_back((int)sCompNode.size());
            int bw = 0;
            std::vector<std::vector<int4>> adj(ni + nb);
            for (int e : compEdges[c]) {
                const int a = ge1[e], b = ge2[e], pa = fixed[a] ? -1 - a : sPos[a], pb = fixed[b] ? -1 - b : sPos[b];
                const int ls = scaleId[e] < 0 ? -1 : (int)(std::lower_bound(sc.begin(), sc.end(), scaleId[e]) - sc.begin());
                if (pa >= 0 && pb >= 0 && pa < ni && pb < ni) bw = std::max(bw, std::abs(pa - pb));
                if (pb >= 0) adj[pb].push_back(make_int4(e, 0, pa, ls));
                if (pa >= 0) adj[pa].push_back(make_int4(e, 1, pb, ls));
                if (ls >= 0) seEnt.push_back(make_int4(e, pa, pb, ls));
            }
            sePtr.push_back((int)seEnt.size());
            for (auto& v : adj) {
                sAdjEnt.insert(sAdjEnt.end(), v.begin(), v.end());
                sAdjPtr.push_back((int)sAdjEnt.size());
            }
            const int nI = 3 * ni, nB = 3 * nb, nS = (int)sc.size(), nT = nB + 4 + nS, w = ni ? std::min(3 * bw + 2, nI - 1) : 0;
            sCompDim.push_back(make_int4(ni, nb, w, nS));
            const size_t need = (size_t)nI * (w + 1 + nT) + (size_t)nT * nT + nI + nB;
            if (need <= (size_t)PG_LDS_DOUBLES) {
                sCompOff.push_back(-1);
                sLdsDoubles = std::max(sLdsDoubles, need);
            } else {
                sCompOff.push_back((long long)scratchDoubles);
                scratchDoubles += need;
            }
            nScalesTotal += nS, nBorderTotal += nb, maxInteriorW = std::max(maxInteriorW, w);
        }
        for (int i = 0; i < N; ++i)
            if (inScaled[i]) nodeSlot[i] = 0;  // the kernel's tail only asks "fixed?" of this array
        compGraph.insert(compGraph.end(), sCompGraph.begin(), sCompGraph.end());
    }
    // (the device is asked for only here: a graph that is refused is refused with or without one)
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || device < 0 || device >= ndev) {
        cs_set_error("%s: no usable HIP device %d (there is no CPU fallback)", fn, device);
        return CS_ERR_NO_DEVICE;
    }
    cs_posegraph* G = new (std::nothrow) cs_posegraph();
    if (!G) {
        cs_set_error("%s: out of memory", fn);
        return CS_ERR_ALLOC;
    }
    G->device = device;
    G->nGraphs = nGraphs, G->nNodes = N, G->nEdges = E, G->nComp = nComp;
    G->ldsBytes = ldsDoubles * sizeof(double);
    G->compGraph = compGraph;
    G->nSComp = nSComp, G->nScales = nScalesTotal, G->nBorder = nBorderTotal, G->maxInteriorW = maxInteriorW;
    G->sLdsBytes = sLdsDoubles * sizeof(double);
    // one device block
    auto pad = [](size_t b) { return (b + 255) & ~(size_t)255; };
    const size_t oCompPtr = 0, oCompNode = oCompPtr + pad(4 * (size_t)(nComp + 1)), oCompW = oCompNode + pad(4 * (size_t)nFree),
                 oCompOff = oCompW + pad(4 * (size_t)nComp), oAdjPtr = oCompOff + pad(8 * (size_t)nComp),
                 oAdjEnt = oAdjPtr + pad(4 * (size_t)(nFree + 1)), oNodeSlot = oAdjEnt + pad(16 * adjEnt.size()),
                 oGe1 = oNodeSlot + pad(4 * (size_t)N), oGe2 = oGe1 + pad(4 * (size_t)E), oSCompPtr = oGe2 + pad(4 * (size_t)E),
                 oSCompNode = oSCompPtr + pad(4 * sCompPtr.size()), oSCompDim = oSCompNode + pad(4 * sCompNode.size()),
                 oSCompOff = oSCompDim + pad(16 * sCompDim.size()), oSAdjPtr = oSCompOff + pad(8 * sCompOff.size()),
                 oSAdjEnt = oSAdjPtr + pad(4 * sAdjPtr.size()), oSePtr = oSAdjEnt + pad(16 * sAdjEnt.size()),
                 oSeEnt = oSePtr + pad(4 * sePtr.size()), oStatus = oSeEnt + pad(16 * seEnt.size()),
                 oScratch = oStatus + pad(4 * (size_t)std::max(nComp + nSComp, 1)), planBytes = oScratch,
                 oStage = oScratch + pad(8 * scratchDoubles), total = oStage + pad(8 * (24 * (size_t)N + 13 * (size_t)E));
    std::vector<char> h(planBytes, 0);
    auto put = [&](size_t off, const void* src, size_t bytes) {
        if (bytes) memcpy(h.data() + off, src, bytes);
    };
    put(oCompPtr, compPtr.data(), 4 * (size_t)(nComp + 1));
    put(oCompNode, compNode.data(), 4 * (size_t)nFree);
    put(oCompW, compW.data(), 4 * (size_t)nComp);
    put(oCompOff, compOff.data(), 8 * (size_t)nComp);
    put(oAdjPtr, adjPtr.data(), 4 * (size_t)(nFree + 1));
    put(oAdjEnt, adjEnt.data(), 16 * adjEnt.size());
    put(oNodeSlot, nodeSlot.data(), 4 * (size_t)N);
    if (anyScaled)  // the scaled edges' rows of edgeR / edgeT are the caller's (MergeInfo::R, t): cs_posegraph_edges_dev skips them
        for (int e = 0; e < E; ++e)
            if (scaleId[e] >= 0) ge1[e] = -1;
    put(oGe1, ge1.data(), 4 * (size_t)E);
    put(oGe2, ge2.data(), 4 * (size_t)E);
    put(oSCompPtr, sCompPtr.data(), 4 * sCompPtr.size());
    put(oSCompNode, sCompNode.data(), 4 * sCompNode.size());
    put(oSCompDim, sCompDim.data(), 16 * sCompDim.size());
    put(oSCompOff, sCompOff.data(), 8 * sCompOff.size());
    put(oSAdjPtr, sAdjPtr.data(), 4 * sAdjPtr.size());
    put(oSAdjEnt, sAdjEnt.data(), 16 * sAdjEnt.size());
    put(oSePtr, sePtr.data(), 4 * sePtr.size());
    put(oSeEnt, seEnt.data(), 16 * seEnt.size());
    hipError_t e = hipSetDevice(device);
    if (e == hipSuccess) e = hipMalloc((void**)&G->dev, total);
    if (e == hipSuccess) e = hipMemcpy(G->dev, h.data(), planBytes, hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        cs_set_error("%s: %s", fn, hipGetErrorString(e));
        if (G->dev) (void)hipFree(G->dev);
        delete G;
        return CS_ERR_HIP;
    }
    PgPlan& p = G->plan;
    p.nComp = nComp, p.nNodes = N, p.nEdges = E;
    p.compPtr = (const int*)(G->dev + oCompPtr);
    p.compNode = (const int*)(G->dev + oCompNode);
    p.compW = (const int*)(G->dev + oCompW);
    p.compOff = (const long long*)(G->dev + oCompOff);
    p.adjPtr = (const int*)(G->dev + oAdjPtr);
    p.adjEnt = (const int4*)(G->dev + oAdjEnt);
    p.nodeSlot = (const int*)(G->dev + oNodeSlot);
    p.ge1 = (const int*)(G->dev + oGe1);
    p.ge2 = (const int*)(G->dev + oGe2);
    p.status = (int*)(G->dev + oStatus);
    p.scratch = (double*)(G->dev + oScratch);
    G->dIn = (double*)(G->dev + oStage);  // staging of the host form: nodeR | nodeT | edgeR | edgeT | newR | newT | edgeS
    PgsPlan& sp = G->splan;
    sp.nComp = nSComp;
    sp.compPtr = (const int*)(G->dev + oSCompPtr);
    sp.compNode = (const int*)(G->dev + oSCompNode);
    sp.compDim = (const int4*)(G->dev + oSCompDim);
    sp.compOff = (const long long*)(G->dev + oSCompOff);
    sp.adjPtr = (const int*)(G->dev + oSAdjPtr);
    sp.adjEnt = (const int4*)(G->dev + oSAdjEnt);
    sp.sePtr = (const int*)(G->dev + oSePtr);
    sp.seEnt = (const int4*)(G->dev + oSeEnt);
    sp.scratch = p.scratch;
    sp.status = p.status + nComp;
    *out = G;
    return CS_OK;
}

extern "C" int cs_posegraph_create(int device, int nGraphs, const int* nodePtr, const int* edgePtr, const unsigned char* fixed,
                                   const int* id1, const int* id2, cs_posegraph** out) {
    return pg_create("cs_posegraph_create", device, nGraphs, nodePtr, edgePtr, fixed, id1, id2, nullptr, out);
}

extern "C" int cs_posegraph_create_scaled(int device, int nGraphs, const int* nodePtr, const int* edgePtr, const unsigned char* fixed,
                                          const int* id1, const int* id2, const int* scaleId, cs_posegraph** out) {
    return pg_create(scaleId ? "cs_posegraph_create_scaled" : "cs_posegraph_create", device, nGraphs, nodePtr, edgePtr, fixed, id1, id2,
                     scaleId, out);
}

extern "C" int cs_posegraph_scaled_counts(const cs_posegraph* g, int* nScales, int* nBorderNodes, int* maxInteriorHalfBandwidth) {
    if (!g) {
        cs_set_error("cs_posegraph_scaled_counts: null handle");
        return CS_ERR_INVALID;
    }
    if (nScales) *nScales = g->nScales;
    if (nBorderNodes) *nBorderNodes = g->nBorder;
    if (maxInteriorHalfBandwidth) *maxInteriorHalfBandwidth = g->maxInteriorW;
    return CS_OK;
}

extern "C" void cs_posegraph_destroy(cs_posegraph* g) {
    if (!g) return;
    (void)hipSetDevice(g->device);
    if (g->dev) (void)hipFree(g->dev);
    delete g;
}

extern "C" int cs_posegraph_counts(const cs_posegraph* g, int* nNodes, int* nEdges, int* nComponents, int* maxHalfBandwidth) {
    if (!g) {
        cs_set_error("cs_posegraph_counts: null handle");
        return CS_ERR_INVALID;
    }
    if (nNodes) *nNodes = g->nNodes;
    if (nEdges) *nEdges = g->nEdges;
    if (nComponents) *nComponents = g->nComp + g->nSComp;
    if (maxHalfBandwidth) {
        std::vector<int> w(g->nComp);
        if (g->nComp) {
            CS_HIP(hipSetDevice(g->device));
            CS_HIP(hipMemcpy(w.data(), g->plan.compW, 4 * (size_t)g->nComp, hipMemcpyDeviceToHost));
        }
        *maxHalfBandwidth = std::max(g->nComp ? *std::max_element(w.begin(), w.end()) : 0, g->maxInteriorW);
    }
    return CS_OK;
}

extern "C" int cs_posegraph_edges_dev(cs_posegraph* g, void* hip_stream, const double* d_nodeR, const double* d_nodeT,
                                      double* d_edgeR, double* d_edgeT) {
    if (!g || (g->nEdges > 0 && (!d_nodeR || !d_nodeT || !d_edgeR || !d_edgeT))) {
        cs_set_error("cs_posegraph_edges_dev: null pointer");
        return CS_ERR_INVALID;
    }
    if (g->nEdges == 0) return CS_OK;
    CS_HIP(hipSetDevice(g->device));
    hipLaunchKernelGGL(k_posegraph_edges, dim3((g->nEdges + 127) / 128), dim3(128), 0, (hipStream_t)hip_stream, g->nEdges, g->plan.ge1,
                       g->plan.ge2, d_nodeR, d_nodeT, d_edgeR, d_edgeT);
    CS_CHECK_LAUNCH();
    return CS_OK;
}

extern "C" int cs_posegraph_set_poses_dev(int device, void* hip_stream, int n, const int* d_nodeIdx, const double* d_R,
                                          const double* d_t, double* d_nodeR, double* d_nodeT) {
    if (n < 0 || (n > 0 && (!d_nodeIdx || !d_R || !d_t || !d_nodeR || !d_nodeT))) {
        cs_set_error("cs_posegraph_set_poses_dev: bad argument");
        return CS_ERR_INVALID;
    }
    if (n == 0) return CS_OK;
    CS_HIP(hipSetDevice(device));
    hipLaunchKernelGGL(k_posegraph_set_poses, dim3((n + 127) / 128), dim3(128), 0, (hipStream_t)hip_stream, n, d_nodeIdx, d_R, d_t,
                       d_nodeR, d_nodeT);
    CS_CHECK_LAUNCH();
    return CS_OK;
}

extern "C" int cs_posegraph_relax_dev(cs_posegraph* g, void* hip_stream, const double* d_nodeR, const double* d_nodeT,
                                      const double* d_edgeR, const double* d_edgeT, double* d_newR, double* d_newT) {
    if (!g || (g->nNodes > 0 && (!d_nodeR || !d_nodeT || !d_newR || !d_newT)) || (g->nEdges > 0 && (!d_edgeR || !d_edgeT))) {
        cs_set_error("cs_posegraph_relax_dev: null pointer");
        return CS_ERR_INVALID;
    }
    if (d_newR == d_nodeR || d_newT == d_nodeT) {
        cs_set_error("cs_posegraph_relax_dev: the new poses must not alias the node poses (free nodes read their fixed neighbours)");
        return CS_ERR_INVALID;
    }
    if (g->nSComp) {
        cs_set_error("cs_posegraph_relax_dev: the handle has uncertain-scale edges, use cs_posegraph_relax_scaled_dev");
        return CS_ERR_INVALID;
    }
    if (g->nNodes == 0) return CS_OK;
    CS_HIP(hipSetDevice(g->device));
    const int grid = g->nComp + (g->nNodes + 63) / 64;
    hipLaunchKernelGGL(k_posegraph_relax, dim3(grid), dim3(64), g->ldsBytes, (hipStream_t)hip_stream, g->plan, d_nodeR, d_nodeT, d_edgeR,
                       d_edgeT, d_newR, d_newT);
    CS_CHECK_LAUNCH();
    return CS_OK;
}

extern "C" int cs_posegraph_relax_scaled_dev(cs_posegraph* g, void* hip_stream, const double* d_nodeR, const double* d_nodeT,
                                             const double* d_edgeR, const double* d_edgeT, double* d_newR, double* d_newT,
                                             double* d_edgeS) {
    if (!g || (g->nNodes > 0 && (!d_nodeR || !d_nodeT || !d_newR || !d_newT)) || (g->nEdges > 0 && (!d_edgeR || !d_edgeT || !d_edgeS))) {
        cs_set_error("cs_posegraph_relax_scaled_dev: null pointer");
        return CS_ERR_INVALID;
    }
    if (d_newR == d_nodeR || d_newT == d_nodeT) {
        cs_set_error("cs_posegraph_relax_scaled_dev: the new poses must not alias the node poses (free nodes read their fixed neighbours)");
        return CS_ERR_INVALID;
    }
    if (g->nNodes == 0) return CS_OK;
    CS_HIP(hipSetDevice(g->device));
    if (g->nEdges) CS_HIP(hipMemsetAsync(d_edgeS, 0, sizeof(double) * (size_t)g->nEdges, (hipStream_t)hip_stream));
    // the plain components and the fixed nodes: the launch of cs_posegraph_relax_dev
    const int grid = g->nComp + (g->nNodes + 63) / 64;
    hipLaunchKernelGGL(k_posegraph_relax, dim3(grid), dim3(64), g->ldsBytes, (hipStream_t)hip_stream, g->plan, d_nodeR, d_nodeT, d_edgeR,
                       d_edgeT, d_newR, d_newT);
    CS_CHECK_LAUNCH();
    if (g->nSComp) {
        hipLaunchKernelGGL(k_posegraph_relax_scaled, dim3(g->nSComp), dim3(PGS_THREADS), g->sLdsBytes, (hipStream_t)hip_stream, g->splan,
                           d_nodeR, d_nodeT, d_edgeR, d_edgeT, d_newR, d_newT, d_edgeS);
        CS_CHECK_LAUNCH();
    }
    return CS_OK;
}

extern "C" int cs_posegraph_status(cs_posegraph* g, void* hip_stream, int* nFailed, int* firstFailedGraph) {
    if (!g) {
        cs_set_error("cs_posegraph_status: null handle");
        return CS_ERR_INVALID;
    }
    if (nFailed) *nFailed = 0;
    if (firstFailedGraph) *firstFailedGraph = -1;
    CS_HIP(hipSetDevice(g->device));
    const int nAll = g->nComp + g->nSComp;
    std::vector<int> st(nAll);
    if (nAll) CS_HIP(hipMemcpyAsync(st.data(), g->plan.status, 4 * (size_t)nAll, hipMemcpyDeviceToHost, (hipStream_t)hip_stream));
    CS_HIP(hipStreamSynchronize((hipStream_t)hip_stream));
    int bad = 0, first = -1, code = 0;
    for (int c = 0; c < nAll; ++c)
        if (st[c]) {
            if (first < 0) first = g->compGraph[c], code = st[c];
            ++bad;
        }
    if (nFailed) *nFailed = bad;
    if (firstFailedGraph) *firstFailedGraph = first;
    if (bad) {
        cs_set_error("pose-graph relaxation: %d component(s) failed, first in graph %d (%s)", bad, first,
                     code == 1   ? "a free node is not constrained by any edge"
                     : code == 3 ? "a scale unknown is not determined: the translations of its edges are zero or dependent"
                                 : "a solved 3x3 block is singular");
        return CS_ERR_NUMERIC;
    }
    return CS_OK;
}

// the status words on the device, for a guard that must not wait for the host (csrc/merge_apply.hip)
void cs_posegraph_status_words(const cs_posegraph* g, const int** d_status, int* n) {
    *d_status = g ? g->plan.status : nullptr;
    *n = g ? g->nComp + g->nSComp : 0;
}

extern "C" int cs_posegraph_relax(cs_posegraph* g, const double* nodeR, const double* nodeT, const double* edgeR,
                                  const double* edgeT, double* newR, double* newT) {
    if (!g || (g->nNodes > 0 && (!nodeR || !nodeT || !newR || !newT)) || (g->nEdges > 0 && (!edgeR || !edgeT))) {
        cs_set_error("cs_posegraph_relax: null pointer");
        return CS_ERR_INVALID;
    }
    if (g->nNodes == 0) return CS_OK;
    CS_HIP(hipSetDevice(g->device));
    const size_t N = g->nNodes, E = g->nEdges, inD = 12 * N + 12 * E;
    double* d = g->dIn;
    hipStream_t s = nullptr;
    // (pageable copies: a few KB each; a pinned staging block would cost more to allocate than these copies take)
    CS_HIP(hipMemcpyAsync(d, nodeR, 9 * N * 8, hipMemcpyHostToDevice, s));
    CS_HIP(hipMemcpyAsync(d + 9 * N, nodeT, 3 * N * 8, hipMemcpyHostToDevice, s));
    if (E) {
        CS_HIP(hipMemcpyAsync(d + 12 * N, edgeR, 9 * E * 8, hipMemcpyHostToDevice, s));
        CS_HIP(hipMemcpyAsync(d + 12 * N + 9 * E, edgeT, 3 * E * 8, hipMemcpyHostToDevice, s));
    }
    int rc = cs_posegraph_relax_dev(g, s, d, d + 9 * N, d + 12 * N, d + 12 * N + 9 * E, d + inD, d + inD + 9 * N);
    if (rc != CS_OK) return rc;
    CS_HIP(hipMemcpyAsync(newR, d + inD, 9 * N * 8, hipMemcpyDeviceToHost, s));
    CS_HIP(hipMemcpyAsync(newT, d + inD + 9 * N, 3 * N * 8, hipMemcpyDeviceToHost, s));
    rc = cs_posegraph_status(g, s, nullptr, nullptr);  // synchronises the stream
    return rc;
}

extern "C" int cs_posegraph_relax_scaled(cs_posegraph* g, const double* nodeR, const double* nodeT, const double* edgeR,
                                         const double* edgeT, double* newR, double* newT, double* edgeS) {
    if (!g || (g->nNodes > 0 && (!nodeR || !nodeT || !newR || !newT)) || (g->nEdges > 0 && (!edgeR || !edgeT || !edgeS))) {
        cs_set_error("cs_posegraph_relax_scaled: null pointer");
        return CS_ERR_INVALID;
    }
    if (g->nNodes == 0) return CS_OK;
    CS_HIP(hipSetDevice(g->device));
    const size_t N = g->nNodes, E = g->nEdges, inD = 12 * N + 12 * E;
    double* d = g->dIn;
    hipStream_t s = nullptr;
    CS_HIP(hipMemcpyAsync(d, nodeR, 9 * N * 8, hipMemcpyHostToDevice, s));
    CS_HIP(hipMemcpyAsync(d + 9 * N, nodeT, 3 * N * 8, hipMemcpyHostToDevice, s));
    if (E) {
        CS_HIP(hipMemcpyAsync(d + 12 * N, edgeR, 9 * E * 8, hipMemcpyHostToDevice, s));
        CS_HIP(hipMemcpyAsync(d + 12 * N + 9 * E, edgeT, 3 * E * 8, hipMemcpyHostToDevice, s));
    }
    int rc = cs_posegraph_relax_scaled_dev(g, s, d, d + 9 * N, d + 12 * N, d + 12 * N + 9 * E, d + inD, d + inD + 9 * N, d + inD + 12 * N);
    if (rc != CS_OK) return rc;
    CS_HIP(hipMemcpyAsync(newR, d + inD, 9 * N * 8, hipMemcpyDeviceToHost, s));
    CS_HIP(hipMemcpyAsync(newT, d + inD + 9 * N, 3 * N * 8, hipMemcpyDeviceToHost, s));
    if (E) CS_HIP(hipMemcpyAsync(edgeS, d + inD + 12 * N, E * 8, hipMemcpyDeviceToHost, s));
    rc = cs_posegraph_status(g, s, nullptr, nullptr);  // synchronises the stream
    return rc;
}

extern "C" int cs_posegraph_after_ba(void* hip_stream, void* rec) {
    const cs_posegraph_after_ba_rec* r = (const cs_posegraph_after_ba_rec*)rec;
    if (!r || !r->g) {
        cs_set_error("cs_posegraph_after_ba: null record");
        return CS_ERR_INVALID;
    }
    int rc = cs_posegraph_set_poses_dev(r->device, hip_stream, r->nCams, r->d_camNode, r->d_Rs, r->d_Ts, r->d_nodeR, r->d_nodeT);
    if (rc == CS_OK) rc = cs_posegraph_relax_dev(r->g, hip_stream, r->d_nodeR, r->d_nodeT, r->d_edgeR, r->d_edgeT, r->d_newR, r->d_newT);
    return rc;
}
