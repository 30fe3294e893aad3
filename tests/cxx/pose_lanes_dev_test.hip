// pose_lanes_dev_test.hip -- the lane exchanges of the intra-camera pose solve's LM step against the forms they replaced, bit for bit,
// on one wave of the device:
//   reduce: cs_reduce_many<N> (coslam_amd/csrc/cs_common.h: lane swaps and DPP) against the select-and-__shfl_xor butterfly kept below,
//           per owner lane, for 1, 2, 3, 7 (the tree's small ends) and every N the library instantiates: 9 (ba.hip), 27, 28, 33, 42
//           (the pose solve and the BA kernels) and 45 (merge_front.hip); 9 and 45 reach it through cs_wave_sum_many_d in the library;
//   solve:  solve66_lanes (coslam_amd/csrc/pose_solve_dev.h: a column per lane) against the entry-per-lane form kept below.
// Prints "pose_lanes ok ..." and returns 0 when every bit agrees.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../coslam_amd/csrc/cs_common.h"
#include "../../coslam_amd/csrc/pose_solve_dev.h"

#define CHECK(call)                                                                      \
    do {                                                                                 \
        hipError_t e_ = (call);                                                          \
        if (e_ != hipSuccess) {                                                          \
            printf("%s: %s (line %d)\n", #call, hipGetErrorString(e_), __LINE__);        \
            return 2;                                                                    \
        }                                                                                \
    } while (0)

void cs_set_error(const char*, ...) {}

// ---- the forms before: every exchange a ds_bpermute ------------------------------------------------------------------------------
template <int M, int DIST>
__device__ __forceinline__ void old_reduce_step(double* v, int lane) {
    if constexpr (DIST >= 1) {
        constexpr int H = (M + 1) / 2;
        const bool up = (lane & DIST) != 0;
#pragma unroll
        for (int t = 0; t < H; ++t) {
            const double lo = v[t];
            const double hi = (H + t < M) ? v[H + t] : 0.0;
            const double recv = cs_shfl_xor_d(up ? lo : hi, DIST);
            v[t] = (up ? hi : lo) + recv;
        }
        old_reduce_step<H, DIST / 2>(v, lane);
    }
}
__device__ __forceinline__ double old_shfl_d(double v, int srcLane) {
    int lo = __shfl(__double2loint(v), srcLane, 64), hi = __shfl(__double2hiint(v), srcLane, 64);
    return __hiloint2double(hi, lo);
}
__device__ __forceinline__ void old_solve66_lanes(double m, int lane, double* param) {   // lane 7 r + j holds M[r][j]
    const int r = lane / 7, j = lane - 7 * r;
    const bool in = r < 6;
#pragma unroll
    for (int c = 0; c < 6; ++c) {
        double best = fabs(cs_readlane_d(m, 7 * c + c));
        int p = c;
#pragma unroll
        for (int rr = c + 1; rr < 6; ++rr) {
            const double v = fabs(cs_readlane_d(m, 7 * rr + c));
            if (v > best) best = v, p = rr;
        }
        const int srcRow = r == c ? p : (r == p ? c : r);
        const double sw = old_shfl_d(m, in ? 7 * srcRow + j : lane);
        m = sw;
        const double d = cs_readlane_d(m, 7 * c + c);
        const double q = m / d;
        if (r == c && j > c) m = q;
        const double f = old_shfl_d(m, in ? 7 * r + c : lane);
        const double pr = old_shfl_d(m, in ? 7 * c + j : lane);
        const double e = m - f * pr;
        if (in && r != c && j > c) m = e;
    }
#pragma unroll
    for (int rr = 0; rr < 6; ++rr) param[rr] = cs_readlane_d(m, 7 * rr + 6);
}

// ---- kernels: one wave per case -----------------------------------------------------------------------------------------------------
template <int N>
__global__ __launch_bounds__(64) void k_reduce(const double* __restrict__ in /* [cases][64][N] */, double* __restrict__ outNew,
                                               double* __restrict__ outOld /* [cases][64] */) {
    const int lane = threadIdx.x;
    const size_t base = ((size_t)blockIdx.x * 64 + lane) * N;
    double a[N], b[N];
#pragma unroll
    for (int q = 0; q < N; ++q) a[q] = b[q] = in[base + q];
    cs_reduce_many<N>(a, lane);
    old_reduce_step<N, 32>(b, lane);
    outNew[(size_t)blockIdx.x * 64 + lane] = a[0];
    outOld[(size_t)blockIdx.x * 64 + lane] = b[0];
}
__global__ __launch_bounds__(64) void k_solve(const double* __restrict__ in /* [cases][6][7] */, double* __restrict__ outNew,
                                              double* __restrict__ outOld /* [cases][6] */) {
    const int lane = threadIdx.x;
    const double* M = in + (size_t)blockIdx.x * 42;
    double pn[6], po[6], col[6];
    const int j = lane < 6 ? lane : 6;   // lanes >= 7 carry column 6 again, as in the pose solve
#pragma unroll
    for (int r = 0; r < 6; ++r) col[r] = M[7 * r + j];
    solve66_lanes(col, lane, pn);
    old_solve66_lanes(lane < 42 ? M[lane] : 0.0, lane, po);
    if (lane == 0) {
        for (int r = 0; r < 6; ++r) outNew[(size_t)blockIdx.x * 6 + r] = pn[r], outOld[(size_t)blockIdx.x * 6 + r] = po[r];
    }
}

// ---- host -----------------------------------------------------------------------------------------------------------------------------
static uint64_t g_s = 12345;
static uint64_t rnd() {  // splitmix64
    uint64_t z = (g_s += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
static double uni() { return (double)(rnd() >> 11) * (1.0 / 9007199254740992.0) * 2.0 - 1.0; }
static double from_bits(uint64_t b) {
    double d;
    memcpy(&d, &b, 8);
    return d;
}

template <int N>
static int run_reduce(long& compared) {
    // case kinds: 0 random, 1 cancelling magnitudes, 2 zeros of either sign, 3 one +inf lane per value, 4 one not-a-number lane per
    // value (a payload of its own), 5 +inf and -inf in two lanes, 6 zeros and one random lane
    const int kinds = 7, reps = 6, cases = kinds * reps;
    std::vector<double> in((size_t)cases * 64 * N);
    for (int cs = 0; cs < cases; ++cs) {
        const int kind = cs % kinds;
        double* x = &in[(size_t)cs * 64 * N];
        for (int l = 0; l < 64; ++l)
            for (int q = 0; q < N; ++q) {
                double v = uni();
                if (kind == 1) v = ldexp(uni(), (int)(rnd() % 120) - 60);
                if (kind == 2) v = (rnd() & 1) ? 0.0 : -0.0;
                if (kind == 6) v = (rnd() & 1) ? 0.0 : -0.0;
                x[(size_t)l * N + q] = v;
            }
        for (int q = 0; q < N; ++q) {
            const int l0 = (int)(rnd() % 64), l1 = (l0 + 1 + (int)(rnd() % 63)) % 64;
            if (kind == 1)   // the two largest addends cancel
                x[(size_t)l0 * N + q] = 0x1p70 * (1 + q), x[(size_t)l1 * N + q] = -0x1p70 * (1 + q);
            if (kind == 3) x[(size_t)l0 * N + q] = from_bits(0x7ff0000000000000ull);
            if (kind == 4) x[(size_t)l0 * N + q] = from_bits(0x7ff8000000000000ull | (0x1000u + q));
            if (kind == 5) x[(size_t)l0 * N + q] = from_bits(0x7ff0000000000000ull), x[(size_t)l1 * N + q] = from_bits(0xfff0000000000000ull);
            if (kind == 6) x[(size_t)l0 * N + q] = uni();
        }
    }
    double *dIn, *dNew, *dOld;
    CHECK(hipMalloc((void**)&dIn, in.size() * 8));
    CHECK(hipMalloc((void**)&dNew, (size_t)cases * 64 * 8));
    CHECK(hipMalloc((void**)&dOld, (size_t)cases * 64 * 8));
    CHECK(hipMemcpy(dIn, in.data(), in.size() * 8, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(k_reduce<N>, dim3(cases), dim3(64), 0, 0, dIn, dNew, dOld);
    CHECK(hipGetLastError());
    CHECK(hipDeviceSynchronize());
    std::vector<double> a((size_t)cases * 64), b((size_t)cases * 64);
    CHECK(hipMemcpy(a.data(), dNew, a.size() * 8, hipMemcpyDeviceToHost));
    CHECK(hipMemcpy(b.data(), dOld, b.size() * 8, hipMemcpyDeviceToHost));
    CHECK(hipFree(dIn));
    CHECK(hipFree(dNew));
    CHECK(hipFree(dOld));
    int owners = 0;
    for (int l = 0; l < 64; ++l) owners += cs_reduce_index<N>(l) >= 0;
    if (owners != N) return printf("reduce<%d>: %d owner lanes\n", N, owners), 1;
    for (int cs = 0; cs < cases; ++cs)
        for (int l = 0; l < 64; ++l) {
            const int q = cs_reduce_index<N>(l);
            if (q < 0) continue;
            ++compared;
            if (memcmp(&a[(size_t)cs * 64 + l], &b[(size_t)cs * 64 + l], 8) != 0)
                return printf("reduce<%d>: case %d (kind %d) value %d in lane %d: %a against %a before\n", N, cs, cs % kinds, q, l,
                              a[(size_t)cs * 64 + l], b[(size_t)cs * 64 + l]), 1;
            if (cs % kinds == 0) {   // (and the total is the total: the serial sum within a loose bound)
                double s = 0;
                for (int k = 0; k < 64; ++k) s += in[((size_t)cs * 64 + k) * N + q];
                if (fabs(s - a[(size_t)cs * 64 + l]) > 1e-12) return printf("reduce<%d>: value %d is not the sum\n", N, q), 1;
            }
        }
    return 0;
}

// the pivot rule on the host, to COUNT which row swaps and ties a system exercises (not a reference for the values)
static void pivots_of(const double* Min, int* swapAt, int* tieAt) {
    double M[6][7];
    memcpy(M, Min, sizeof(M));
    for (int c = 0; c < 6; ++c) {
        int p = c;
        double best = fabs(M[c][c]);
        bool tie = false;
        for (int r = c + 1; r < 6; ++r) {
            if (fabs(M[r][c]) > best) best = fabs(M[r][c]), p = r, tie = false;
            else if (fabs(M[r][c]) == best) tie = true;
        }
        if (!(best > 0)) return;   // singular or not a number: nothing further to count
        if (p != c) ++swapAt[c];
        if (tie) ++tieAt[c];
        for (int j = 0; j < 7; ++j) std::swap(M[c][j], M[p][j]);
        const double d = M[c][c];
        for (int j = c + 1; j < 7; ++j) M[c][j] /= d;
        for (int r = 0; r < 6; ++r)
            if (r != c)
                for (int j = c + 1; j < 7; ++j) M[r][j] -= M[r][c] * M[c][j];
    }
}

static int run_solve(long& compared) {
    std::vector<double> in;
    auto push = [&](const double (&M)[6][7]) { in.insert(in.end(), &M[0][0], &M[0][0] + 42); };
    double M[6][7];
    // 1. what the LM step solves: J^T J + lambda I with lambda = 1e-3 ... 1e18, J^T r on the right
    for (int rep = 0; rep < 8; ++rep)
        for (int e = -3; e <= 18; ++e) {
            double J[9][6];
            for (auto& row : J)
                for (int j = 0; j < 6; ++j) row[j] = uni() * (j < 3 ? 300.0 : 3.0);
            for (int r = 0; r < 6; ++r) {
                for (int j = 0; j < 6; ++j) {
                    double s = 0;
                    for (auto& row : J) s += row[r] * row[j];
                    M[r][j] = s;
                }
                M[r][r] += pow(10.0, e);
                M[r][6] = uni() * 50;
            }
            push(M);
        }
    // 2. the largest entry of a column off the diagonal: dominant permutations (every cyclic shift and random ones) over noise,
    //    and plain dense matrices
    for (int rep = 0; rep < 120; ++rep) {
        int perm[6] = {0, 1, 2, 3, 4, 5};
        if (rep < 5) {
            for (int r = 0; r < 6; ++r) perm[r] = (r + rep + 1) % 6;
        } else {
            for (int r = 5; r > 0; --r) std::swap(perm[r], perm[rnd() % (r + 1)]);
        }
        for (int r = 0; r < 6; ++r)
            for (int j = 0; j < 7; ++j) M[r][j] = uni() * (rep % 3 == 2 ? 1.0 : 0.05) + (j < 6 && rep % 3 != 2 && perm[j] == r ? (uni() > 0 ? 7.0 : -7.0) : 0.0);
        push(M);
    }
    // 3. ties in the pivot search: small integers of either sign (some of these are singular: zero pivots, infinities, not-a-number)
    for (int rep = 0; rep < 120; ++rep) {
        for (int r = 0; r < 6; ++r)
            for (int j = 0; j < 7; ++j) M[r][j] = (double)((int)(rnd() % 5) - 2) + (rep % 2 && r == j ? 0.0 : (rnd() % 3 == 0 ? 1.0 : 0.0));
        if (rep % 4 == 0)
            for (int r = 0; r < 6; ++r) M[r][0] = (r & 1) ? -3.0 : 3.0;   // all six tie at step 0: row 0 wins
        push(M);
    }
    //    ... and a tie made for every step: 2 I with column c = +-3 from row c down (all of them tie, row c wins and stays), or with
    //    a smaller entry in row c (rows c + 1 ... tie, row c + 1 wins and is swapped in)
    for (int c = 0; c < 5; ++c)
        for (int variant = 0; variant < 2; ++variant) {
            for (int r = 0; r < 6; ++r) {
                for (int j = 0; j < 6; ++j) M[r][j] = r == j ? 2.0 : 0.0;
                M[r][6] = uni();
                if (r >= c) M[r][c] = (r & 1) ? -3.0 : 3.0;
            }
            if (variant) M[c][c] = 1.0;
            push(M);
        }
    // 4. a zero pivot: column c all zero from row c down; and one not-a-number entry at every position
    for (int c = 0; c < 6; ++c) {
        for (int r = 0; r < 6; ++r)
            for (int j = 0; j < 7; ++j) M[r][j] = (j == c && r >= c) ? 0.0 : uni() + (r == j ? 4.0 : 0.0);
        push(M);
    }
    for (int pos = 0; pos < 42; ++pos) {
        for (int r = 0; r < 6; ++r)
            for (int j = 0; j < 7; ++j) M[r][j] = uni() + (r == j ? 2.0 : 0.0);
        M[pos / 7][pos % 7] = from_bits(0x7ff8000000000000ull | (0x2000u + pos));
        push(M);
    }
    const int cases = (int)(in.size() / 42);
    int swapAt[6] = {0}, tieAt[6] = {0};
    for (int cs = 0; cs < cases; ++cs) pivots_of(&in[(size_t)cs * 42], swapAt, tieAt);
    for (int c = 0; c < 5; ++c)
        if (!swapAt[c] || !tieAt[c]) return printf("solve: step %d has %d swaps and %d ties among the cases\n", c, swapAt[c], tieAt[c]), 1;
    double *dIn, *dNew, *dOld;
    CHECK(hipMalloc((void**)&dIn, in.size() * 8));
    CHECK(hipMalloc((void**)&dNew, (size_t)cases * 6 * 8));
    CHECK(hipMalloc((void**)&dOld, (size_t)cases * 6 * 8));
    CHECK(hipMemcpy(dIn, in.data(), in.size() * 8, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(k_solve, dim3(cases), dim3(64), 0, 0, dIn, dNew, dOld);
    CHECK(hipGetLastError());
    CHECK(hipDeviceSynchronize());
    std::vector<double> a((size_t)cases * 6), b((size_t)cases * 6);
    CHECK(hipMemcpy(a.data(), dNew, a.size() * 8, hipMemcpyDeviceToHost));
    CHECK(hipMemcpy(b.data(), dOld, b.size() * 8, hipMemcpyDeviceToHost));
    CHECK(hipFree(dIn));
    CHECK(hipFree(dNew));
    CHECK(hipFree(dOld));
    // Every unknown that is a number (infinities included) has the same 64 bits in both forms.  An unknown that is not-a-number must
    // be not-a-number in both, and that is all: its sign and payload are not the source's to decide.  Once a column holds more than one
    // not-a-number, f * pr and m - f * pr meet two of them with different signs, the hardware hands on the one in its FIRST operand,
    // and which operand that is the compiler chooses instruction by instruction (v_mul_f64 s, v here, v_mul_f64 v, s two lines on, in
    // one and the same unrolled loop); the negation it folds into the add's second operand flips the sign of what passes through it.
    // The last 42 systems hold ONE not-a-number each and nothing that could make another (no infinity, no zero pivot): whatever
    // meets there carries that one payload, so there only the sign is left out and the other 63 bits must agree.
    int nans = 0;
    for (int cs = 0; cs < cases; ++cs) {
        for (int r = 0; r < 6; ++r) {
            const double x = a[(size_t)cs * 6 + r], y = b[(size_t)cs * 6 + r];
            ++compared;
            if (x != x && y != y) {
                ++nans;
                if (cs >= cases - 42) {
                    uint64_t bx, by;
                    memcpy(&bx, &x, 8), memcpy(&by, &y, 8);
                    if ((bx ^ by) << 1) return printf("solve: system %d unknown %d: payloads %016llx against %016llx before\n", cs, r, (unsigned long long)bx, (unsigned long long)by), 1;
                }
                continue;
            }
            if (memcmp(&x, &y, 8) != 0) return printf("solve: system %d unknown %d: %a against %a before\n", cs, r, x, y), 1;
        }
        // (and the solution solves: the residual of the first kind of system)
        if (cs < 8 * 22) {
            const double* S = &in[(size_t)cs * 42];
            for (int r = 0; r < 6; ++r) {
                double s = -S[7 * r + 6], scale = fabs(S[7 * r + 6]);
                for (int j = 0; j < 6; ++j) s += S[7 * r + j] * a[(size_t)cs * 6 + j], scale += fabs(S[7 * r + j] * a[(size_t)cs * 6 + j]);
                if (!(fabs(s) <= 1e-9 * scale)) return printf("solve: system %d row %d residual %g\n", cs, r, s), 1;
            }
        }
    }
    if (nans < 42) return printf("solve: only %d unknowns are not-a-number: the cases with one in the matrix give at least one each\n", nans), 1;
    printf("solve: %d systems, %d unknowns not-a-number in both forms, swaps per step %d %d %d %d %d, ties per step %d %d %d %d %d\n", cases, nans, swapAt[0], swapAt[1], swapAt[2], swapAt[3],
           swapAt[4], tieAt[0], tieAt[1], tieAt[2], tieAt[3], tieAt[4]);
    return 0;
}

int main(int argc, char** argv) {
    const bool reduce = argc < 2 || !strcmp(argv[1], "reduce"), solve = argc < 2 || !strcmp(argv[1], "solve");
    long nr = 0, ns = 0;
    if (reduce) {
        int rc = run_reduce<1>(nr);
        if (!rc) rc = run_reduce<2>(nr);
        if (!rc) rc = run_reduce<3>(nr);
        if (!rc) rc = run_reduce<7>(nr);
        if (!rc) rc = run_reduce<9>(nr);
        if (!rc) rc = run_reduce<27>(nr);
        if (!rc) rc = run_reduce<28>(nr);
        if (!rc) rc = run_reduce<33>(nr);
        if (!rc) rc = run_reduce<42>(nr);
        if (!rc) rc = run_reduce<45>(nr);
        if (rc) return rc;
    }
    if (solve) {
        int rc = run_solve(ns);
        if (rc) return rc;
    }
    printf("pose_lanes ok reduce %ld solve %ld\n", nr, ns);
    return 0;
}
