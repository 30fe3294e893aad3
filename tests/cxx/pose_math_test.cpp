// pose_math_test.cpp -- the structured perturbed rotations of the intra-camera pose solve against the product they replace, on the
// host, byte for byte (coslam_amd/csrc/pose_math.h; compile with -ffp-contract=off):
//   1. so3_exp(eps e_k) is I + eps [e_k]x: entries 1, +0, +eps, -eps with eps = 1e-8 = 0x1.5798ee2308c3ap-27;
//   2. mat33_perturbed<k>(R) == mat33AB(R, so3_exp(eps e_k)) on random rotations, random matrices with entries of either sign,
//      tiny (subnormal products) and huge ones;
//   3. the documented exception: an entry of R that is -0 may come out as -0 where the full product gives +0 (equal as numbers).
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "../../coslam_amd/csrc/pose_math.h"

static uint64_t g_s = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() {  // splitmix64
    uint64_t z = (g_s += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
static double uni() { return (double)(rnd() >> 11) * (1.0 / 9007199254740992.0) * 2.0 - 1.0; }  // [-1, 1)

static bool same_bytes(const double* a, const double* b, int n) { return memcmp(a, b, sizeof(double) * n) == 0; }

static void perturbed(int k, const double* R, double* C) {
    if (k == 0) mat33_perturbed<0>(R, C);
    else if (k == 1) mat33_perturbed<1>(R, C);
    else mat33_perturbed<2>(R, C);
}

int main() {
    const double eps = 1e-8;
    {
        const double want = 0x1.5798ee2308c3ap-27;
        if (memcmp(&eps, &want, 8) != 0) return printf("eps is not 0x1.5798ee2308c3ap-27\n"), 1;
    }
    double dR[3][9];
    for (int k = 0; k < 3; ++k) {
        double w[3] = {0, 0, 0};
        w[k] = 1e-8;
        so3_exp(w, dR[k]);
        const int p = (k + 1) % 3, q = (k + 2) % 3;
        double want[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};   // I + eps [e_k]x: [e_k]x[q][p] = 1, [e_k]x[p][q] = -1
        want[3 * q + p] = eps;
        want[3 * p + q] = -eps;
        if (!same_bytes(dR[k], want, 9)) return printf("so3_exp(eps e_%d) is not I + eps [e_%d]x\n", k, k), 1;
    }
    long n = 0;
    auto check = [&](const double* R, const char* what) -> bool {
        for (int k = 0; k < 3; ++k) {
            double full[9], fast[9];
            mat33AB(R, dR[k], full);
            perturbed(k, R, fast);
            ++n;
            if (!same_bytes(full, fast, 9)) {
                printf("%s: k = %d differs\n", what, k);
                for (int i = 0; i < 9; ++i) printf("  R %a full %a structured %a\n", R[i], full[i], fast[i]);
                return false;
            }
        }
        return true;
    };
    for (int it = 0; it < 200000; ++it) {
        double R[9], w[3] = {3 * uni(), 3 * uni(), 3 * uni()};
        so3_exp(w, R);   // a rotation
        if (!check(R, "rotation")) return 1;
        for (int i = 0; i < 9; ++i) R[i] = uni();
        if (!check(R, "signed")) return 1;
        // magnitudes over the whole exponent range, subnormals and values next to the overflow threshold included, either sign
        for (int i = 0; i < 9; ++i) {
            uint64_t b = rnd();
            const uint64_t e = (b >> 52) & 0x7ff;
            if (e == 0x7ff) b &= ~(1ull << 52);   // keep it finite
            if ((b << 1) == 0) b |= 1;            // no zero of either sign here (case 3 below)
            memcpy(&R[i], &b, 8);
        }
        if (!check(R, "whole range")) return 1;
        const double s = (it & 1) ? 0x1p-1040 : 0x1p+1000;
        for (int i = 0; i < 9; ++i) R[i] = s * uni() + (uni() > 0 ? s : -s) * 0x1p-30;
        if (!check(R, (it & 1) ? "tiny" : "huge")) return 1;
    }
    // +0 entries anywhere: still the same bytes
    for (int it = 0; it < 20000; ++it) {
        double R[9];
        for (int i = 0; i < 9; ++i) R[i] = (rnd() & 1) ? 0.0 : uni();
        if (!check(R, "+0 entries")) return 1;
    }
    // -0 entries: equal as numbers, and where the bytes differ the full product has +0 and the structured one -0
    for (int it = 0; it < 20000; ++it) {
        double R[9];
        for (int i = 0; i < 9; ++i) R[i] = (rnd() & 1) ? -0.0 : ((rnd() & 1) ? 0.0 : uni());
        for (int k = 0; k < 3; ++k) {
            double full[9], fast[9];
            mat33AB(R, dR[k], full);
            perturbed(k, R, fast);
            for (int i = 0; i < 9; ++i) {
                const double pz = 0.0, nz = -0.0;
                const bool same = memcmp(&full[i], &fast[i], 8) == 0;
                const bool documented = memcmp(&full[i], &pz, 8) == 0 && memcmp(&fast[i], &nz, 8) == 0;
                if (!same && !documented) return printf("-0 entries: k = %d entry %d: full %a structured %a\n", k, i, full[i], fast[i]), 1;
            }
        }
    }
    printf("pose_math ok %ld\n", n);
    return 0;
}
