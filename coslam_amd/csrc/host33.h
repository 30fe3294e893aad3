// host33.h -- the library's host-side 3 x 3 inverse.
#pragma once

#include <cmath>

// mat33Inv is un-vendored: the library's definition is Gauss-Jordan elimination with partial pivoting on [K | I], the one the reference
// drivers are linked with (so that F agrees with them to the bit)
inline bool cs_host_inv33(const double* K, double* iK) {
    double M[3][6];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) M[i][j] = K[3 * i + j], M[i][3 + j] = i == j ? 1.0 : 0.0;
    for (int c = 0; c < 3; ++c) {
        int piv = c;
        for (int r = c + 1; r < 3; ++r)
            if (fabs(M[r][c]) > fabs(M[piv][c])) piv = r;
        if (piv != c)
            for (int j = 0; j < 6; ++j) {
                const double t = M[c][j];
                M[c][j] = M[piv][j], M[piv][j] = t;
            }
        const double d = M[c][c];
        if (!(d != 0) || d != d) return false;
        for (int j = 0; j < 6; ++j) M[c][j] /= d;
        for (int r = 0; r < 3; ++r) {
            if (r == c) continue;
            const double f = M[r][c];
            if (f == 0.0) continue;
            for (int j = 0; j < 6; ++j) M[r][j] -= f * M[c][j];
        }
    }
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) iK[3 * i + j] = M[i][3 + j];
    return true;
}
