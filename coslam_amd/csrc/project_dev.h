// project_dev.h -- the library's one definition of project(K, R, t, M, m): m = pi(K (R M + t)) (a LibVisualSLAM function that is not in the
// reference tree).  f64, a fixed operation order (the library is built with -ffp-contract=off); the pixel is (u / w, v / w).
#pragma once

#include "cs_common.h"

// everything one (camera, point) pair needs of the projection: u, v, w and J = d project / dM
struct PuProj {
    double u, v, w, J[6];
};
__device__ __forceinline__ PuProj pu_project(const double* __restrict__ K, const double* __restrict__ R, const double* __restrict__ t,
                                             const double M[3]) {
    PuProj q;
    const double X = ((R[0] * M[0] + R[1] * M[1]) + R[2] * M[2]) + t[0];
    const double Y = ((R[3] * M[0] + R[4] * M[1]) + R[5] * M[2]) + t[1];
    const double Z = ((R[6] * M[0] + R[7] * M[1]) + R[8] * M[2]) + t[2];
    double KR[9];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) KR[3 * i + j] = (K[3 * i] * R[j] + K[3 * i + 1] * R[3 + j]) + K[3 * i + 2] * R[6 + j];
    q.u = (K[0] * X + K[1] * Y) + K[2] * Z;
    q.v = (K[3] * X + K[4] * Y) + K[5] * Z;
    q.w = (K[6] * X + K[7] * Y) + K[8] * Z;
    const double ww = q.w * q.w;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        q.J[j] = (KR[j] * q.w - q.u * KR[6 + j]) / ww;
        q.J[3 + j] = (KR[3 + j] * q.w - q.v * KR[6 + j]) / ww;
    }
    return q;
}
