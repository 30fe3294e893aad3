// pose_math.h -- the rotation arithmetic of the intra-camera pose solve (pose.hip), host and device: a plain C++ compiler can
// include it (tests/cxx/pose_math_test.cpp does).  FMA contraction is OFF for everything below: by the pragma under clang (hipcc), by
// -ffp-contract=off on the command line of any other compiler.
#pragma once

#include <cmath>

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

#if defined(__HIPCC__)
#define CS_PM_FN static __host__ __device__ __forceinline__
#define CS_PM_UNROLL _Pragma("unroll")
#else
#define CS_PM_FN static inline
#define CS_PM_UNROLL
#endif

CS_PM_FN void so3_exp(const double w[3], double R[9]) {  // SL_IntraCamPose.cpp:10-39
    double theta = sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2]);
    if (theta == 0) {
        R[0] = 1, R[1] = 0, R[2] = 0, R[3] = 0, R[4] = 1, R[5] = 0, R[6] = 0, R[7] = 0, R[8] = 1;
        return;
    }
    double hw0 = w[0] / theta, hw1 = w[1] / theta, hw2 = w[2] / theta;
    double st, ct;
    if (theta < 0.5) {
        // an LM step's rotation is a fraction of a degree: sin and cos from their Taylor series (truncation below 2^-56 of the
        // value for theta < 0.5; the library's routines carry a range reduction for arguments this never sees)
        const double x2 = theta * theta;
        double ps = 1.0 / 355687428096000.0;   // 1 / 17!
        ps = ps * x2 - 1.0 / 1307674368000.0;
        ps = ps * x2 + 1.0 / 6227020800.0;
        ps = ps * x2 - 1.0 / 39916800.0;
        ps = ps * x2 + 1.0 / 362880.0;
        ps = ps * x2 - 1.0 / 5040.0;
        ps = ps * x2 + 1.0 / 120.0;
        ps = ps * x2 - 1.0 / 6.0;
        st = theta + theta * (x2 * ps);
        double pc = 1.0 / 20922789888000.0;    // 1 / 16!
        pc = pc * x2 - 1.0 / 87178291200.0;
        pc = pc * x2 + 1.0 / 479001600.0;
        pc = pc * x2 - 1.0 / 3628800.0;
        pc = pc * x2 + 1.0 / 40320.0;
        pc = pc * x2 - 1.0 / 720.0;
        pc = pc * x2 + 1.0 / 24.0;
        const double c = 1.0 - (0.5 * x2 - x2 * x2 * pc);   // cos(theta), rounded: the reference forms 1 - cos(theta) from that (:20)
        ct = 1 - c;
    } else {
        st = sin(theta);
        ct = 1 - cos(theta);
    }
    double hw0hw0 = hw0 * hw0, hw0hw1 = hw0 * hw1, hw0hw2 = hw0 * hw2;
    double hw1hw1 = hw1 * hw1, hw1hw2 = hw1 * hw2, hw2hw2 = hw2 * hw2;
    R[0] = -ct * hw1hw1 - ct * hw2hw2 + 1;
    R[1] = ct * hw0hw1 - st * hw2;
    R[2] = st * hw1 + ct * hw0hw2;
    R[3] = st * hw2 + ct * hw0hw1;
    R[4] = -ct * hw0hw0 - ct * hw2hw2 + 1;
    R[5] = ct * hw1hw2 - st * hw0;
    R[6] = ct * hw0hw2 - st * hw1;
    R[7] = st * hw0 + ct * hw1hw2;
    R[8] = -ct * hw0hw0 - ct * hw1hw1 + 1;
}

CS_PM_FN void mat33AB(const double* A, const double* B, double* C) {
    double T[9];
    CS_PM_UNROLL
    for (int i = 0; i < 3; ++i)
        CS_PM_UNROLL
        for (int j = 0; j < 3; ++j) T[3 * i + j] = A[3 * i] * B[j] + A[3 * i + 1] * B[3 + j] + A[3 * i + 2] * B[6 + j];
    CS_PM_UNROLL
    for (int i = 0; i < 9; ++i) C[i] = T[i];
}

// R exp(eps e_k) for the forward differences' eps = 1e-8 (SL_IntraCamPose.cpp:57-59), from the factor's structure: so3_exp gives
// exp(eps e_k) = I + eps [e_k]x exactly (sin(eps) rounds to eps, cos(eps) to 1; entries 1, +0, +eps, -eps), so with p = k + 1 and
// q = k + 2 (mod 3) the product mat33AB(R, exp(eps e_k)) is column k of R copied, column p = R[.][p] + R[.][q] eps and column
// q = R[.][p] (-eps) + R[.][q]: the zero terms mat33AB adds change nothing, and the association of the remaining two is mat33AB's.
// Bit for bit the same product (tests/cxx/pose_math_test.cpp), with ONE exception: where mat33AB adds a +0 term to an entry of R
// that is -0 it gives +0 and this gives -0 (a copied column, or the first addend of a sum whose other addend is -0 too).
template <int K>
CS_PM_FN void mat33_perturbed(const double* R, double* C) {
    constexpr int P = (K + 1) % 3, Q = (K + 2) % 3;
    const double eps = 1e-8;
    CS_PM_UNROLL
    for (int i = 0; i < 3; ++i) {
        const double rp = R[3 * i + P], rq = R[3 * i + Q];
        C[3 * i + K] = R[3 * i + K];
        C[3 * i + P] = rp + rq * eps;
        C[3 * i + Q] = rp * (-eps) + rq;
    }
}
