// triangulate_dev.h -- the library's one definition of the multi-view triangulation pieces (un-vendored LibVisualSLAM: getCameraCenter,
// normPoint, triangulateMultiView, getTriangulateCovMat; definitions in DESIGN.md 3.9, the oracle's operation for operation).  Shared by the
// map-point kernels of poseupdate.hip and merge_apply.hip.  f64, a fixed operation order (the library is built with -ffp-contract=off).
#pragma once

#include "cs_common.h"

// the 3x3 normal equations of triangulateMultiView, summed view by view: N = {n00, n01, n02, n11, n12, n22}
struct UpNormalEq {
    double N[6], g[3];
};
__device__ __forceinline__ void up_add_view(UpNormalEq& E, const double* __restrict__ iK, const double* __restrict__ R,
                                            const double* __restrict__ t, double mx, double my) {
    const double w = (iK[6] * mx + iK[7] * my) + iK[8];
    const double x = ((iK[0] * mx + iK[1] * my) + iK[2]) / w, y = ((iK[3] * mx + iK[4] * my) + iK[5]) / w;  // normPoint
    const double a0[3] = {R[0] - x * R[6], R[1] - x * R[7], R[2] - x * R[8]}, a1[3] = {R[3] - y * R[6], R[4] - y * R[7], R[5] - y * R[8]};
    const double b0 = x * t[2] - t[0], b1 = y * t[2] - t[1];
    E.N[0] = E.N[0] + (a0[0] * a0[0] + a1[0] * a1[0]);
    E.N[1] = E.N[1] + (a0[0] * a0[1] + a1[0] * a1[1]);
    E.N[2] = E.N[2] + (a0[0] * a0[2] + a1[0] * a1[2]);
    E.N[3] = E.N[3] + (a0[1] * a0[1] + a1[1] * a1[1]);
    E.N[4] = E.N[4] + (a0[1] * a0[2] + a1[1] * a1[2]);
    E.N[5] = E.N[5] + (a0[2] * a0[2] + a1[2] * a1[2]);
#pragma unroll
    for (int q = 0; q < 3; ++q) E.g[q] = E.g[q] + (a0[q] * b0 + a1[q] * b1);
}
__device__ __forceinline__ void up_add_jtj(double* S, const double* J) {
    S[0] = S[0] + (J[0] * J[0] + J[3] * J[3]);
    S[1] = S[1] + (J[0] * J[1] + J[3] * J[4]);
    S[2] = S[2] + (J[0] * J[2] + J[3] * J[5]);
    S[3] = S[3] + (J[1] * J[1] + J[4] * J[4]);
    S[4] = S[4] + (J[1] * J[2] + J[4] * J[5]);
    S[5] = S[5] + (J[2] * J[2] + J[5] * J[5]);
}
// symmetric 3x3 {n00, n01, n02, n11, n12, n22}: cofactors (same order) and the determinant
__device__ __forceinline__ double up_sym33_cof(const double* N, double* c) {
    c[0] = N[3] * N[5] - N[4] * N[4];
    c[1] = N[2] * N[4] - N[1] * N[5];
    c[2] = N[1] * N[4] - N[2] * N[3];
    c[3] = N[0] * N[5] - N[2] * N[2];
    c[4] = N[1] * N[2] - N[0] * N[4];
    c[5] = N[0] * N[3] - N[1] * N[1];
    return (N[0] * c[0] + N[1] * c[1]) + N[2] * c[2];
}
// getCameraCenter: C = -R^T t
__device__ __forceinline__ void up_cam_center(const double* __restrict__ R, const double* __restrict__ t, double* C) {
#pragma unroll
    for (int i = 0; i < 3; ++i) C[i] = -((R[i] * t[0] + R[3 + i] * t[1]) + R[6 + i] * t[2]);
}
