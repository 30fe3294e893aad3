// merge_front.hip -- the front of MergeCameraGroup::matchMergableCameras, gfx950 (reference src/app/SL_MergeCameraGroup.cpp:360-378):
// matchSURFPoints -> computeEMat -> getMatchedPts, from key points + descriptors to what the merge matcher takes per candidate camera pair
// (a JOB): E, the seed rows, surfNum, ematOk.  DESIGN.md 3.25.  matchSurf / estimateEMat / evaluateEMat are un-vendored LibVisualSLAM: the
// definitions are OURS, restated in numpy by tests/mergefront_ref.py.
//
//   k_mf_valid    per camera: a point takes part iff its key point is finite and within 1e6 px and its descriptor is finite (a wave per point)
//   k_mf_match    matchSurf's search: 64 rows of camera 1 per workgroup (descriptors transposed in LDS), camera 2's descriptors tiled through
//                 LDS 32 at a time, direct f32 differences, best / second best per row in registers, four waves share a tile's columns and
//                 merge; the ratio / maxDist test; the one-to-one rule as an integer atomic minimum of {f32 bits of d1, i} per column
//   k_mf_collect  the rows that hold their column, in ascending i (ordered compaction: ballot + prefix), and their point rows
//   k_mf_gather   the point rows of a caller's match list (the computeEMat-shaped entry)
//   k_mf_hyp      one hypothesis per 16-lane group: counter-based sample of 8 matches, the normalised eight-point solve in f64 with every
//                 matrix in LDS (lane r owns row r of the 9 x 9 Jacobi; nothing is indexed in registers: no scratch)
//   k_mf_score    one workgroup per hypothesis, lanes over matches, ballot / popcount; the best as ONE integer atomic maximum of {count, ~h}
//   k_mf_refit    one workgroup per job: <= 4 rounds of the eight-point solve over all inliers (A^T A: per-lane partial sums, the wave
//                 butterfly of cs_common.h, four wave totals added in a fixed order), re-score, keep iff the count did not fall -- decided on
//                 the device; then newMatches, the seed rows and the job's result record
// Results are the same bits from run to run: every reduction has a fixed shape, the only atomics are integer minima / maxima / sums.
#include <cfloat>
#include <climits>
#include <cmath>
#include <vector>

#include "cs_common.h"
#include "dev_arena.h"
#include "host33.h"

#pragma clang fp contract(off)

namespace {

constexpr int MF_MAX_CAMS = 16, MF_MAX_PTS = 32768, MF_MAX_DIM = 128, MF_MAX_HYP = 65536;
constexpr int MF_DRAWS = 64;                    // draws a hypothesis may spend on its 8 distinct indices
constexpr int MF_SWEEPS9 = 10, MF_SWEEPS3 = 10;  // the Jacobi stopping rule: a fixed number of cyclic sweeps
constexpr int MF_REFIT_ROUNDS = 4;
constexpr int MF_ROWS = 64, MF_COLS = 32, MF_T = 256;

typedef unsigned long long mf_u64;

struct MfJob {
    const double *p1, *p2;   // [n][2] pixels
    const float *d1, *d2;    // [n][dim]
    const int *v1, *v2;      // [n] validity (k_mf_valid); NULL in the computeEMat-shaped entry: every point takes part
    int n1, n2, out, pad;    // out: the job's row of the outputs and the k of the sample generator
    double iK1[9], iK2[9];
};

struct MfArgs {
    const MfJob* jobs;       // [nb], slot order
    int maxPts, dim, maxHyp, nHyp;
    float ratio, maxDist;
    double maxEpiErr;
    int minInlierNum;
    mf_u64 seed;
    // per batch slot
    int* rowJ;               // [slots][maxPts]
    float* rowD;             // [slots][maxPts]
    mf_u64* colBest;         // [slots][maxPts]
    double* pix;             // [slots][maxPts][4] = x1, y1, x2, y2 of every match
    double* nrm;             // [slots][maxPts][4] = the same through iK
    unsigned char* flagTmp;  // [slots][maxPts]
    int* hypSample;          // [slots][maxHyp][8]
    int* hypCount;           // [slots][maxHyp]
    double* hypE;            // [slots][maxHyp][9]
    mf_u64* best;            // [slots]
    // per job
    int* matches;            // [256][maxPts][2]
    float* dist;             // [256][maxPts]
    int* count;              // [256]
    unsigned char* inlierFlag;  // [256][maxPts]
    double* seeds;           // [256][maxPts][4]
    int* newMatches;         // [256][maxPts][2]
    cs_merge_front_result* results;  // [256]
};

// LDS traffic between the lanes of ONE wave: the hardware keeps a wave's LDS operations in order, the compiler must as well
__device__ __forceinline__ void mf_wsync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// ---- the sample generator: a 64-bit mix of (seed, k, h, draw); tests/mergefront_ref.py spells out the same ----
__device__ __forceinline__ unsigned mf_rand_hi(mf_u64 seed, int k, int h, int draw) {
    const mf_u64 c = ((mf_u64)(unsigned)k << 40) | ((mf_u64)(unsigned)h << 8) | (mf_u64)(unsigned)draw;
    mf_u64 z = seed + (c + 1ull) * 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    z ^= z >> 31;
    return (unsigned)(z >> 32);
}

// F = iK2^T E iK1 (getFMat(iK1, iK2, E)): T = iK2^T E, F = T iK1
__device__ __forceinline__ void mf_fmat(const double* E, const double* iK1, const double* iK2, double* F) {
    double T[9];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) T[3 * i + j] = (iK2[i] * E[j] + iK2[3 + i] * E[3 + j]) + iK2[6 + i] * E[6 + j];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) F[3 * i + j] = (T[3 * i] * iK1[j] + T[3 * i + 1] * iK1[3 + j]) + T[3 * i + 2] * iK1[6 + j];
}
// epipolarError(F, p2, p1): the distance of p2 from the line F (p1, 1); a line without direction gives NaN or inf: no inlier
__device__ __forceinline__ double mf_epi(const double* F, double x1, double y1, double x2, double y2) {
    const double l0 = (F[0] * x1 + F[1] * y1) + F[2];
    const double l1 = (F[3] * x1 + F[4] * y1) + F[5];
    const double l2 = (F[6] * x1 + F[7] * y1) + F[8];
    return fabs((l0 * x2 + l1 * y2) + l2) / sqrt(l0 * l0 + l1 * l1);
}

// ---- the eight-point solve behind A^T A, one 16-lane group, every matrix in LDS ----
struct MfWs {
    double A[81], V[81];   // A^T A and its eigenvectors
    double D[72];          // the 8 x 9 design matrix of a minimal sample
    double P[32];          // the 8 sampled rows {x1, y1, x2, y2} (normalised image coordinates)
    double B[9], W[9];     // the 3 x 3 one-sided Jacobi: B = E W, columns of B orthogonal at the end
    double E[9];
    int smp[8];
    int ok, pad;
};

// element (a, i) of the Hartley transform T = [s 0 -s cx; 0 s -s cy; 0 0 1]
__device__ __forceinline__ double mf_t(double s, double cx, double cy, int a, int i) {
    if (a == 2) return i == 2 ? 1.0 : 0.0;
    if (i == a) return s;
    if (i == 2) return a == 0 ? -(s * cx) : -(s * cy);
    return 0.0;
}

// cyclic Jacobi on the symmetric 9 x 9 A (rows p < q in order, MF_SWEEPS9 sweeps), V <- V J; lane r < 9 owns row r
__device__ void mf_jacobi9(double* A, double* V, int r) {
    for (int sw = 0; sw < MF_SWEEPS9; ++sw)
        for (int p = 0; p < 8; ++p)
            for (int q = p + 1; q < 9; ++q) {
                const double apq = A[9 * p + q];
                if (apq == 0.0) continue;   // (the same for every lane of the group)
                const double app = A[9 * p + p], aqq = A[9 * q + q];
                const double th = (aqq - app) / (2.0 * apq);
                const double t = (th >= 0.0 ? 1.0 : -1.0) / (fabs(th) + sqrt(th * th + 1.0));
                const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
                double arp = 0, arq = 0, vrp = 0, vrq = 0;
                if (r < 9) arp = A[9 * r + p], arq = A[9 * r + q], vrp = V[9 * r + p], vrq = V[9 * r + q];
                mf_wsync();
                if (r < 9) {
                    if (r == p) {
                        A[9 * p + p] = app - t * apq, A[9 * p + q] = 0.0;
                    } else if (r == q) {
                        A[9 * q + q] = aqq + t * apq, A[9 * q + p] = 0.0;
                    } else {
                        const double np = c * arp - s * arq, nq = s * arp + c * arq;
                        A[9 * r + p] = np, A[9 * p + r] = np, A[9 * r + q] = nq, A[9 * q + r] = nq;
                    }
                    V[9 * r + p] = c * vrp - s * vrq, V[9 * r + q] = s * vrp + c * vrq;
                }
                mf_wsync();
            }
}

// From A^T A (ws.A, with ws.V = I) and the two Hartley transforms to ws.E: the eigenvector of the smallest eigenvalue (the first of equal
// diagonal entries), de-normalised (T2^T F T1), projected onto the essential manifold by a one-sided 3 x 3 Jacobi SVD (the two largest
// singular values to 1, the smallest -- the first of equals -- to 0), unit Frobenius norm.  -> false: no model (E = 0).  Group-uniform.
__device__ bool mf_solve(MfWs& ws, int r, double s1, double cx1, double cy1, double s2, double cx2, double cy2) {
    mf_jacobi9(ws.A, ws.V, r);
    int m = 0;
    double lo = ws.A[0];
    for (int k = 1; k < 9; ++k) {
        const double d = ws.A[10 * k];
        if (d < lo) lo = d, m = k;
    }
    if (r < 9) {
        const int i = r / 3, j = r - 3 * i;
        double e = 0.0;
        for (int a = 0; a < 3; ++a)
            for (int b = 0; b < 3; ++b) e += (mf_t(s2, cx2, cy2, a, i) * ws.V[9 * (3 * a + b) + m]) * mf_t(s1, cx1, cy1, b, j);
        ws.B[r] = e, ws.W[r] = i == j ? 1.0 : 0.0;
    }
    mf_wsync();
    for (int sw = 0; sw < MF_SWEEPS3; ++sw)
        for (int p = 0; p < 2; ++p)
            for (int q = p + 1; q < 3; ++q) {
                double al = 0, be = 0, ga = 0;
                for (int k = 0; k < 3; ++k) {
                    const double bp = ws.B[3 * k + p], bq = ws.B[3 * k + q];
                    al += bp * bp, be += bq * bq, ga += bp * bq;
                }
                if (ga == 0.0) continue;
                const double ze = (be - al) / (2.0 * ga);
                const double t = (ze >= 0.0 ? 1.0 : -1.0) / (fabs(ze) + sqrt(ze * ze + 1.0));
                const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
                double bp = 0, bq = 0, wp = 0, wq = 0;
                if (r < 3) bp = ws.B[3 * r + p], bq = ws.B[3 * r + q], wp = ws.W[3 * r + p], wq = ws.W[3 * r + q];
                mf_wsync();
                if (r < 3) {
                    ws.B[3 * r + p] = c * bp - s * bq, ws.B[3 * r + q] = s * bp + c * bq;
                    ws.W[3 * r + p] = c * wp - s * wq, ws.W[3 * r + q] = s * wp + c * wq;
                }
                mf_wsync();
            }
    double nc[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) nc[c] = sqrt((ws.B[c] * ws.B[c] + ws.B[3 + c] * ws.B[3 + c]) + ws.B[6 + c] * ws.B[6 + c]);
    const int drop = (nc[1] < nc[0]) ? ((nc[2] < nc[1]) ? 2 : 1) : ((nc[2] < nc[0]) ? 2 : 0);
    const double na = drop == 0 ? nc[1] : nc[0], nb = drop == 2 ? nc[1] : nc[2];
    const bool ok = na > 0.0 && nb > 0.0 && na < DBL_MAX && nb < DBL_MAX;
    if (r < 9) {
        const int i = r / 3, j = r - 3 * i;
        const int ca = drop == 0 ? 1 : 0, cb = drop == 2 ? 1 : 2;
        const double e = (ws.B[3 * i + ca] / na) * ws.W[3 * j + ca] + (ws.B[3 * i + cb] / nb) * ws.W[3 * j + cb];
        ws.E[r] = ok ? e * 0.70710678118654752440 : 0.0;
    }
    mf_wsync();
    return ok;
}

// ---- validity of every point of every camera ----
struct MfValidArgs {
    const double* pts[MF_MAX_CAMS];
    const float* desc[MF_MAX_CAMS];
    int n[MF_MAX_CAMS];
    int* valid;   // [nCams][maxPts]
    int maxPts, dim;
};
__global__ __launch_bounds__(MF_T) void k_mf_valid(MfValidArgs A) {
    const int c = blockIdx.y, i = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (i >= A.n[c]) return;   // (wave-uniform)
    bool ok = true;
    for (int d = lane; d < A.dim; d += 64) ok = ok && fabsf(A.desc[c][(size_t)i * A.dim + d]) <= FLT_MAX;
    const double x = A.pts[c][2 * (size_t)i], y = A.pts[c][2 * (size_t)i + 1];
    ok = ok && fabs(x) < 1.0e6 && fabs(y) < 1.0e6;
    const bool all = __ballot(!ok) == 0;
    if (lane == 0) A.valid[(size_t)c * A.maxPts + i] = all ? 1 : 0;
}

// ---- matchSurf's search ----
__global__ __launch_bounds__(MF_T) void k_mf_match(MfArgs A) {
    const MfJob& J = A.jobs[blockIdx.y];
    const int n1 = J.n1, n2 = J.n2, dim = A.dim, i0 = blockIdx.x * MF_ROWS;
    if (i0 >= n1) return;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    __shared__ float rowT[MF_MAX_DIM][MF_ROWS + 1];
    __shared__ __attribute__((aligned(16))) float colT[MF_MAX_DIM][MF_COLS + 4];
    __shared__ int colV[MF_COLS];
    __shared__ float mD1[4][64], mD2[4][64];
    __shared__ int mJ1[4][64];
    for (int idx = tid; idx < MF_ROWS * dim; idx += MF_T) {
        const int r = idx / dim, d = idx - r * dim;
        rowT[d][r] = i0 + r < n1 ? J.d1[(size_t)(i0 + r) * dim + d] : 0.0f;
    }
    const float inf = __builtin_huge_valf();
    float d1 = inf, d2 = inf;
    int j1 = -1;
    for (int j0 = 0; j0 < n2; j0 += MF_COLS) {
        __syncthreads();
        for (int idx = tid; idx < MF_COLS * dim; idx += MF_T) {
            const int c = idx / dim, d = idx - c * dim;
            colT[d][c] = j0 + c < n2 ? J.d2[(size_t)(j0 + c) * dim + d] : 0.0f;
        }
        if (tid < MF_COLS) colV[tid] = j0 + tid < n2 ? J.v2[j0 + tid] : 0;
        __syncthreads();
#pragma unroll
        for (int g = 0; g < 2; ++g) {
            const int c0 = w * 8 + g * 4;
            float a0 = 0, a1 = 0, a2 = 0, a3 = 0;
            for (int d = 0; d < dim; ++d) {
                const float a = rowT[d][lane];
                const float4 b = *(const float4*)&colT[d][c0];
                const float e0 = a - b.x, e1 = a - b.y, e2 = a - b.z, e3 = a - b.w;
                a0 += e0 * e0, a1 += e1 * e1, a2 += e2 * e2, a3 += e3 * e3;
            }
            const float acc[4] = {a0, a1, a2, a3};
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const float dd = colV[c0 + u] ? sqrtf(acc[u]) : inf;
                if (dd < d1) d2 = d1, d1 = dd, j1 = j0 + c0 + u;
                else if (dd < d2) d2 = dd;
            }
        }
    }
    mD1[w][lane] = d1, mD2[w][lane] = d2, mJ1[w][lane] = j1;
    __syncthreads();
    if (w != 0) return;
    for (int v = 1; v < 4; ++v) {   // the waves' columns interleave: equal distances go to the lowest j
        const float b1 = mD1[v][lane], b2 = mD2[v][lane];
        const int bj = mJ1[v][lane];
        if (b1 < d1 || (b1 == d1 && bj >= 0 && bj < j1)) {
            d2 = d1 < b2 ? d1 : b2, d1 = b1, j1 = bj;
        } else if (b1 < d2) {
            d2 = b1;
        }
    }
    const int i = i0 + lane;
    if (i >= n1) return;
    const size_t sb = (size_t)blockIdx.y * A.maxPts;
    const bool acc = J.v1[i] != 0 && j1 >= 0 && d1 < A.maxDist && d1 < A.ratio * d2;
    A.rowJ[sb + i] = acc ? j1 : -1, A.rowD[sb + i] = d1;
    if (acc) atomicMin(&A.colBest[sb + j1], ((mf_u64)__float_as_uint(d1) << 32) | (mf_u64)(unsigned)i);
}

// the point rows of match `pos` of slot: pixels and normalised image coordinates (x^ = iK (x, y, 1), divided by its third component)
__device__ __forceinline__ void mf_point_rows(const MfArgs& A, const MfJob& J, size_t slotBase, int pos, int i, int j) {
    double px[4], nr[4];
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    if ((unsigned)i < (unsigned)J.n1 && (unsigned)j < (unsigned)J.n2) {
        px[0] = J.p1[2 * (size_t)i], px[1] = J.p1[2 * (size_t)i + 1], px[2] = J.p2[2 * (size_t)j], px[3] = J.p2[2 * (size_t)j + 1];
#pragma unroll
        for (int v = 0; v < 2; ++v) {
            const double* K = v ? J.iK2 : J.iK1;
            const double x = px[2 * v], y = px[2 * v + 1];
            const double h0 = (K[0] * x + K[1] * y) + K[2], h1 = (K[3] * x + K[4] * y) + K[5], h2 = (K[6] * x + K[7] * y) + K[8];
            nr[2 * v] = h0 / h2, nr[2 * v + 1] = h1 / h2;
        }
    } else {
#pragma unroll
        for (int v = 0; v < 4; ++v) px[v] = nan, nr[v] = nan;   // a match outside the cameras' points: never an inlier, never read
    }
    double4* P = (double4*)A.pix + slotBase + pos;
    double4* Q = (double4*)A.nrm + slotBase + pos;
    *P = make_double4(px[0], px[1], px[2], px[3]);
    *Q = make_double4(nr[0], nr[1], nr[2], nr[3]);
}

__global__ __launch_bounds__(MF_T) void k_mf_collect(MfArgs A) {
    const MfJob& J = A.jobs[blockIdx.x];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, n1 = J.n1;
    const size_t sb = (size_t)blockIdx.x * A.maxPts, ob = (size_t)J.out * A.maxPts;
    __shared__ int sWave[4], sBase;
    if (tid == 0) sBase = 0;
    __syncthreads();
    for (int c0 = 0; c0 < n1; c0 += MF_T) {
        const int i = c0 + tid;
        int j = -1;
        float d = 0;
        if (i < n1) {
            j = A.rowJ[sb + i], d = A.rowD[sb + i];
            if (j >= 0 && A.colBest[sb + j] != (((mf_u64)__float_as_uint(d) << 32) | (mf_u64)(unsigned)i)) j = -1;
        }
        const mf_u64 m = __ballot(j >= 0);
        if (lane == 0) sWave[w] = __popcll(m);
        __syncthreads();
        int pos = sBase + __popcll(m & ((1ull << lane) - 1));
        for (int v = 0; v < w; ++v) pos += sWave[v];
        if (j >= 0) {
            A.matches[2 * (ob + pos)] = i, A.matches[2 * (ob + pos) + 1] = j, A.dist[ob + pos] = d;
            mf_point_rows(A, J, sb, pos, i, j);
        }
        __syncthreads();
        if (tid == 0) sBase += (sWave[0] + sWave[1]) + (sWave[2] + sWave[3]);
        __syncthreads();
    }
    if (tid == 0) A.count[J.out] = sBase;
}

__global__ __launch_bounds__(MF_T) void k_mf_gather(MfArgs A) {
    const MfJob& J = A.jobs[blockIdx.y];
    const int n = A.count[J.out], m = blockIdx.x * MF_T + threadIdx.x;
    if (m >= n) return;
    const size_t ob = (size_t)J.out * A.maxPts;
    mf_point_rows(A, J, (size_t)blockIdx.y * A.maxPts, m, A.matches[2 * (ob + m)], A.matches[2 * (ob + m) + 1]);
}

// ---- hypotheses ----
__global__ __launch_bounds__(64) void k_mf_hyp(MfArgs A) {
    const MfJob& J = A.jobs[blockIdx.y];
    const int lane = threadIdx.x, g = lane >> 4, r = lane & 15, h = blockIdx.x * 4 + g;
    __shared__ MfWs sWs[4];
    MfWs& ws = sWs[g];
    if (h >= A.nHyp) return;   // (a whole group leaves: the in-wave syncs are no hardware barrier)
    const int n = A.count[J.out];
    const size_t sb = (size_t)blockIdx.y * A.maxPts, hb = (size_t)blockIdx.y * A.maxHyp + h;
    if (r == 0) {
        int got = 0;
        if (n >= 8)
            for (int draw = 0; draw < MF_DRAWS && got < 8; ++draw) {
                const int idx = (int)(((mf_u64)mf_rand_hi(A.seed, J.out, h, draw) * (mf_u64)(unsigned)n) >> 32);
                bool seen = false;
                for (int k = 0; k < got; ++k) seen = seen || ws.smp[k] == idx;
                if (!seen) ws.smp[got++] = idx;
            }
        ws.ok = got == 8;
    }
    mf_wsync();
    if (!ws.ok) {   // the draws ran out (or fewer than 8 matches): the hypothesis scores 0
        if (r < 8) A.hypSample[8 * hb + r] = -1;
        if (r < 9) A.hypE[9 * hb + r] = 0.0;
        return;
    }
    if (r < 8) {
        const double4 p = ((const double4*)A.nrm)[sb + ws.smp[r]];
        ws.P[4 * r] = p.x, ws.P[4 * r + 1] = p.y, ws.P[4 * r + 2] = p.z, ws.P[4 * r + 3] = p.w;
        A.hypSample[8 * hb + r] = ws.smp[r];
    }
    mf_wsync();
    // Hartley: centroid, mean distance sqrt(2); every lane the same sums in the same order
    double c[4] = {0, 0, 0, 0};
    for (int k = 0; k < 8; ++k) c[0] += ws.P[4 * k], c[1] += ws.P[4 * k + 1], c[2] += ws.P[4 * k + 2], c[3] += ws.P[4 * k + 3];
    c[0] /= 8.0, c[1] /= 8.0, c[2] /= 8.0, c[3] /= 8.0;
    double m1 = 0, m2 = 0;
    for (int k = 0; k < 8; ++k) {
        const double ax = ws.P[4 * k] - c[0], ay = ws.P[4 * k + 1] - c[1], bx = ws.P[4 * k + 2] - c[2], by = ws.P[4 * k + 3] - c[3];
        m1 += sqrt(ax * ax + ay * ay), m2 += sqrt(bx * bx + by * by);
    }
    m1 /= 8.0, m2 /= 8.0;
    bool ok = m1 > 0.0 && m2 > 0.0 && m1 < DBL_MAX && m2 < DBL_MAX;
    const double s1 = 1.4142135623730951 / m1, s2 = 1.4142135623730951 / m2;
    if (ok) {
        if (r < 8) {
            const double x1 = s1 * (ws.P[4 * r] - c[0]), y1 = s1 * (ws.P[4 * r + 1] - c[1]);
            const double x2 = s2 * (ws.P[4 * r + 2] - c[2]), y2 = s2 * (ws.P[4 * r + 3] - c[3]);
            double* D = ws.D + 9 * r;
            D[0] = x2 * x1, D[1] = x2 * y1, D[2] = x2, D[3] = y2 * x1, D[4] = y2 * y1, D[5] = y2, D[6] = x1, D[7] = y1, D[8] = 1.0;
        }
        mf_wsync();
        if (r < 9)
            for (int b = 0; b < 9; ++b) {
                double s = 0.0;
                for (int k = 0; k < 8; ++k) s += ws.D[9 * k + r] * ws.D[9 * k + b];
                ws.A[9 * r + b] = s, ws.V[9 * r + b] = r == b ? 1.0 : 0.0;
            }
        mf_wsync();
        ok = mf_solve(ws, r, s1, c[0], c[1], s2, c[2], c[3]);
    }
    if (r < 9) A.hypE[9 * hb + r] = ok ? ws.E[r] : 0.0;
}

// ---- scoring: evaluateEMat's count of every hypothesis, and the best ----
__global__ __launch_bounds__(MF_T) void k_mf_score(MfArgs A) {
    const MfJob& J = A.jobs[blockIdx.y];
    const int h = blockIdx.x, tid = threadIdx.x, n = A.count[J.out];
    const size_t sb = (size_t)blockIdx.y * A.maxPts, hb = (size_t)blockIdx.y * A.maxHyp + h;
    __shared__ int sCnt;
    if (tid == 0) sCnt = 0;
    __syncthreads();
    double E[9], F[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) E[k] = A.hypE[9 * hb + k];
    mf_fmat(E, J.iK1, J.iK2, F);
    int cnt = 0;
    for (int m0 = 0; m0 < n; m0 += MF_T) {
        const int m = m0 + tid;
        bool in = false;
        if (m < n) {
            const double4 p = ((const double4*)A.pix)[sb + m];
            in = mf_epi(F, p.x, p.y, p.z, p.w) < A.maxEpiErr;
        }
        cnt += __popcll(__ballot(in));
    }
    if ((tid & 63) == 0 && cnt) atomicAdd(&sCnt, cnt);
    __syncthreads();
    if (tid == 0) {
        A.hypCount[hb] = sCnt;
        atomicMax(&A.best[blockIdx.y], ((mf_u64)(unsigned)sCnt << 32) | (mf_u64)(~(unsigned)h));
    }
}

// ---- the best hypothesis' inliers, the local refit, newMatches and seeds ----
__device__ __forceinline__ double mf_block_sum(double v, double* red) {   // red [4]; the four wave totals in a fixed order
    v = cs_wave_sum_d(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return (red[0] + red[1]) + (red[2] + red[3]);
}
// evaluateEMat over all n matches: flags, count, sum of the inliers' errors
__device__ __forceinline__ void mf_evaluate(const MfArgs& A, const MfJob& J, size_t sb, int n, const double* E, unsigned char* flag, int* sInt,
                                            double* red, int& count, double& errSum) {
    double F[9], e[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) e[k] = E[k];
    mf_fmat(e, J.iK1, J.iK2, F);
    const int tid = threadIdx.x;
    int cnt = 0;
    double sum = 0.0;
    for (int m0 = 0; m0 < n; m0 += MF_T) {
        const int m = m0 + tid;
        bool in = false;
        if (m < n) {
            const double4 p = ((const double4*)A.pix)[sb + m];
            const double err = mf_epi(F, p.x, p.y, p.z, p.w);
            in = err < A.maxEpiErr;
            if (in) sum += err;
            flag[m] = in ? 1 : 0;
        }
        cnt += __popcll(__ballot(in));
    }
    __syncthreads();
    if ((tid & 63) == 0) sInt[tid >> 6] = cnt;
    errSum = mf_block_sum(sum, red);
    count = (sInt[0] + sInt[1]) + (sInt[2] + sInt[3]);
    __syncthreads();
}

__global__ __launch_bounds__(MF_T) void k_mf_refit(MfArgs A) {
    const MfJob& J = A.jobs[blockIdx.x];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, n = A.count[J.out];
    const size_t sb = (size_t)blockIdx.x * A.maxPts, ob = (size_t)J.out * A.maxPts;
    __shared__ MfWs ws;
    __shared__ double sE[9], red[4], red45[4][45];
    __shared__ int sInt[4], sOk, sBase;
    unsigned char* const cur = A.inlierFlag + ob;
    unsigned char* const tmp = A.flagTmp + sb;
    cs_merge_front_result* const R = A.results + J.out;
    const mf_u64 bk = A.best[blockIdx.x];
    const int bestH = (int)(~(unsigned)bk), bestCnt = (int)(bk >> 32);
    if (n < 8) {
        if (tid == 0) {
            R->surfNum = n, R->ematOk = 0, R->inlierNum = 0, R->rounds = 0, R->bestHyp = -1, R->flags = CS_MERGE_FRONT_TOO_FEW, R->epiErr = 0.0;
            for (int k = 0; k < 9; ++k) R->E[k] = 0.0;
        }
        for (int m = tid; m < n; m += MF_T) cur[m] = 0;
        return;
    }
    if (tid < 9) sE[tid] = A.hypE[9 * ((size_t)blockIdx.x * A.maxHyp + bestH) + tid];
    __syncthreads();
    int count;
    double errSum;
    mf_evaluate(A, J, sb, n, sE, cur, sInt, red, count, errSum);
    int rounds = 0;
    for (int round = 0; round < MF_REFIT_ROUNDS && count >= 8; ++round) {
        // Hartley over the current inliers
        double s4[4] = {0, 0, 0, 0};
        for (int m = tid; m < n; m += MF_T)
            if (cur[m]) {
                const double4 p = ((const double4*)A.nrm)[sb + m];
                s4[0] += p.x, s4[1] += p.y, s4[2] += p.z, s4[3] += p.w;
            }
        double c[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) c[k] = mf_block_sum(s4[k], red) / (double)count;
        double q1 = 0, q2 = 0;
        for (int m = tid; m < n; m += MF_T)
            if (cur[m]) {
                const double4 p = ((const double4*)A.nrm)[sb + m];
                const double ax = p.x - c[0], ay = p.y - c[1], bx = p.z - c[2], by = p.w - c[3];
                q1 += sqrt(ax * ax + ay * ay), q2 += sqrt(bx * bx + by * by);
            }
        const double m1 = mf_block_sum(q1, red) / (double)count, m2 = mf_block_sum(q2, red) / (double)count;
        if (!(m1 > 0.0 && m2 > 0.0 && m1 < DBL_MAX && m2 < DBL_MAX)) break;
        const double s1 = 1.4142135623730951 / m1, s2 = 1.4142135623730951 / m2;
        // A^T A over all inliers: per-lane partial sums of the 45 upper entries, the wave butterfly, the wave totals in a fixed order
        double acc[45];
#pragma unroll
        for (int k = 0; k < 45; ++k) acc[k] = 0.0;
        for (int m = tid; m < n; m += MF_T)
            if (cur[m]) {
                const double4 p = ((const double4*)A.nrm)[sb + m];
                const double x1 = s1 * (p.x - c[0]), y1 = s1 * (p.y - c[1]), x2 = s2 * (p.z - c[2]), y2 = s2 * (p.w - c[3]);
                const double D[9] = {x2 * x1, x2 * y1, x2, y2 * x1, y2 * y1, y2, x1, y1, 1.0};
                int k = 0;
#pragma unroll
                for (int a = 0; a < 9; ++a)
#pragma unroll
                    for (int b = a; b < 9; ++b) acc[k++] += D[a] * D[b];
            }
        cs_wave_sum_many_d<45>(acc);
#pragma unroll
        for (int k = 0; k < 45; ++k)
            if (lane == 0) red45[w][k] = acc[k];
        __syncthreads();
        if (tid < 81) {
            const int a = tid / 9, b = tid - 9 * a, lo = a < b ? a : b, hi = a < b ? b : a;
            const int k = lo * 9 - lo * (lo - 1) / 2 + (hi - lo);
            ws.A[tid] = (red45[0][k] + red45[1][k]) + (red45[2][k] + red45[3][k]);
            ws.V[tid] = a == b ? 1.0 : 0.0;
        }
        __syncthreads();
        if (tid < 16) {
            const bool ok = mf_solve(ws, tid, s1, c[0], c[1], s2, c[2], c[3]);
            if (tid == 0) sOk = ok ? 1 : 0;
        }
        __syncthreads();
        if (!sOk) break;
        int count2;
        double errSum2;
        mf_evaluate(A, J, sb, n, ws.E, tmp, sInt, red, count2, errSum2);
        if (count2 < count) break;   // kept iff the count did not fall; otherwise the previous E stands
        if (tid < 9) sE[tid] = ws.E[tid];
        for (int m = tid; m < n; m += MF_T) cur[m] = tmp[m];
        count = count2, errSum = errSum2, ++rounds;
        __syncthreads();
    }
    // newMatches and the seed rows: the inliers in match order
    if (tid == 0) sBase = 0;
    __syncthreads();
    for (int m0 = 0; m0 < n; m0 += MF_T) {
        const int m = m0 + tid;
        const bool in = m < n && cur[m] != 0;
        const mf_u64 bal = __ballot(in);
        if (lane == 0) sInt[w] = __popcll(bal);
        __syncthreads();
        int pos = sBase + __popcll(bal & ((1ull << lane) - 1));
        for (int v = 0; v < w; ++v) pos += sInt[v];
        if (in) {
            ((double4*)A.seeds)[ob + pos] = ((const double4*)A.pix)[sb + m];
            A.newMatches[2 * (ob + pos)] = A.matches[2 * (ob + m)], A.newMatches[2 * (ob + pos) + 1] = A.matches[2 * (ob + m) + 1];
        }
        __syncthreads();
        if (tid == 0) sBase += (sInt[0] + sInt[1]) + (sInt[2] + sInt[3]);
        __syncthreads();
    }
    if (tid == 0) {
        R->surfNum = n, R->inlierNum = count, R->ematOk = count >= A.minInlierNum ? 1 : 0, R->rounds = rounds, R->bestHyp = bestH;
        R->flags = bestCnt == 0 ? CS_MERGE_FRONT_NO_MODEL : 0;
        R->epiErr = count > 0 ? errSum / (double)count : 0.0;
        for (int k = 0; k < 9; ++k) R->E[k] = sE[k];
    }
}

}  // namespace

struct cs_merge_front {
    int device, nCams, maxPts, dim, maxJobs, maxHyp;
    char* base;
    size_t bytes;
    cs_merge_front_buffers b;
    int* valid;      // [nCams][maxPts]
    MfJob* jobs;     // [maxJobs]
    MfArgs args;     // the tables (jobs and the call's parameters are set per launch)
    CsStage stage;
};

// the device block: per camera, per batch slot, per hypothesis of a slot, per job
static void mf_layout(cs_merge_front* mf, CsArena& ar) {
    const size_t nS = (size_t)mf->maxJobs * mf->maxPts, nH = (size_t)mf->maxJobs * mf->maxHyp, nJ = CS_MERGE_FRONT_MAX_JOBS, nO = nJ * mf->maxPts;
    MfArgs& A = mf->args;
    ar.take(mf->valid, (size_t)mf->nCams * mf->maxPts), ar.take(mf->jobs, mf->maxJobs);
    ar.take(A.rowJ, nS), ar.take(A.rowD, nS), ar.take(A.colBest, nS), ar.take(A.pix, nS * 4), ar.take(A.nrm, nS * 4), ar.take(A.flagTmp, nS);
    ar.take(A.hypSample, nH * 8), ar.take(A.hypCount, nH), ar.take(A.hypE, nH * 9), ar.take(A.best, mf->maxJobs);
    ar.take(A.matches, nO * 2), ar.take(A.dist, nO), ar.take(A.count, nJ), ar.take(A.inlierFlag, nO), ar.take(A.seeds, nO * 4);
    ar.take(A.newMatches, nO * 2), ar.take(A.results, nJ);
}

extern "C" cs_merge_front* cs_merge_front_create(int device, int nCams, int maxPts, int dimDesc, int maxJobs, int maxHyp) {
    if (nCams < 1 || nCams > MF_MAX_CAMS || maxPts < 1 || maxPts > MF_MAX_PTS || dimDesc < 1 || dimDesc > MF_MAX_DIM || maxJobs < 1 ||
        maxJobs > CS_MERGE_FRONT_MAX_JOBS || maxHyp < 1 || maxHyp > MF_MAX_HYP) {
        cs_set_error("cs_merge_front_create: bad argument (nCams %d of 1..%d, maxPts %d of 1..%d, dimDesc %d of 1..%d, maxJobs %d of 1..%d, maxHyp %d of 1..%d)",
                     nCams, MF_MAX_CAMS, maxPts, MF_MAX_PTS, dimDesc, MF_MAX_DIM, maxJobs, CS_MERGE_FRONT_MAX_JOBS, maxHyp, MF_MAX_HYP);
        return nullptr;
    }
    cs_merge_front* mf = new cs_merge_front();
    mf->device = device, mf->nCams = nCams, mf->maxPts = maxPts, mf->dim = dimDesc, mf->maxJobs = maxJobs, mf->maxHyp = maxHyp;
    MfArgs& A = mf->args;
    memset(&A, 0, sizeof(A));
    if (!cs_arena_alloc(device, mf->base, mf->bytes, [mf](CsArena& ar) { mf_layout(mf, ar); })) {
        cs_set_error("cs_merge_front_create: %zu bytes of device memory: %s", mf->bytes, hipGetErrorString(hipGetLastError()));
        delete mf;
        return nullptr;
    }
    A.maxPts = maxPts, A.dim = dimDesc, A.maxHyp = maxHyp;
    cs_merge_front_buffers& B = mf->b;
    B.matches = A.matches, B.dist = A.dist, B.count = A.count, B.inlierFlag = A.inlierFlag, B.seeds = A.seeds, B.newMatches = A.newMatches;
    B.results = A.results, B.hypSample = A.hypSample, B.hypCount = A.hypCount, B.hypE = A.hypE, B.pix = A.pix, B.valid = mf->valid;
    B.nCams = nCams, B.maxPts = maxPts, B.dimDesc = dimDesc, B.maxJobs = maxJobs, B.maxHyp = maxHyp;
    return mf;
}

extern "C" void cs_merge_front_destroy(cs_merge_front* mf) {
    if (!mf) return;
    if (mf->base) {
        (void)hipSetDevice(mf->device);
        mf->stage.drain();   // (an upload of the last call may still read its staging copy)
        (void)hipFree(mf->base);
    }
    delete mf;
}

namespace {

struct MfParams {
    float ratio, maxDist;
    int nRansac;
    double maxEpiErr;
    int minInlierNum;
    mf_u64 seed;
};

// the tables of a call, checked: -> the jobs of all batches (slot order inside a batch), before anything is enqueued
int mf_check(const char* who, cs_merge_front* mf, const cs_merge_front_cam* cams, int nJobs, const cs_merge_front_job* jobs, int maxJobs,
             bool needDesc, const MfParams* P, std::vector<MfJob>& out) {
    if (!mf || !cams || nJobs < 0 || (nJobs > 0 && !jobs)) {
        cs_set_error("%s: null handle or table", who);
        return CS_ERR_INVALID;
    }
    if (nJobs > maxJobs) {
        cs_set_error("%s: %d jobs of at most %d", who, nJobs, maxJobs);
        return CS_ERR_INVALID;
    }
    if (P && (P->nRansac < 1 || P->nRansac > mf->maxHyp)) {
        cs_set_error("%s: nRansac %d of 1..%d (the handle's maxHyp)", who, P->nRansac, mf->maxHyp);
        return CS_ERR_INVALID;
    }
    double iK[MF_MAX_CAMS][9];
    for (int c = 0; c < mf->nCams; ++c) {
        if (cams[c].n < 0 || cams[c].n > mf->maxPts) {
            cs_set_error("%s: camera %d: %d points, the handle holds %d", who, c, cams[c].n, mf->maxPts);
            return CS_ERR_INVALID;
        }
        if (!cams[c].K || (cams[c].n > 0 && (!cams[c].pts || (needDesc && !cams[c].desc)))) {
            cs_set_error("%s: camera %d: null pts / desc / K", who, c);
            return CS_ERR_INVALID;
        }
        if (!cs_host_inv33(cams[c].K, iK[c])) {
            cs_set_error("%s: camera %d: singular K", who, c);
            return CS_ERR_INVALID;
        }
    }
    out.resize((size_t)nJobs);
    for (int k = 0; k < nJobs; ++k) {
        const int a = jobs[k].iCam, b = jobs[k].jCam;
        if (a < 0 || a >= mf->nCams || b < 0 || b >= mf->nCams || a == b) {
            cs_set_error("%s: job %d: cameras %d / %d of %d", who, k, a, b, mf->nCams);
            return CS_ERR_INVALID;
        }
        MfJob& J = out[k];
        memset(&J, 0, sizeof(J));
        J.p1 = cams[a].pts, J.p2 = cams[b].pts, J.d1 = cams[a].desc, J.d2 = cams[b].desc;
        J.v1 = mf->valid + (size_t)a * mf->maxPts, J.v2 = mf->valid + (size_t)b * mf->maxPts;
        J.n1 = cams[a].n, J.n2 = cams[b].n, J.out = k;
        memcpy(J.iK1, iK[a], sizeof(J.iK1)), memcpy(J.iK2, iK[b], sizeof(J.iK2));
    }
    return CS_OK;
}

MfArgs mf_args(const cs_merge_front* mf, const MfParams& P) {
    MfArgs A = mf->args;
    A.jobs = mf->jobs, A.nHyp = P.nRansac, A.ratio = P.ratio, A.maxDist = P.maxDist, A.maxEpiErr = P.maxEpiErr;
    A.minInlierNum = P.minInlierNum, A.seed = P.seed;
    return A;
}

int mf_valid(cs_merge_front* mf, hipStream_t s, const cs_merge_front_cam* cams) {
    MfValidArgs V;
    memset(&V, 0, sizeof(V));
    int nMax = 0;
    for (int c = 0; c < mf->nCams; ++c) V.pts[c] = cams[c].pts, V.desc[c] = cams[c].desc, V.n[c] = cams[c].n, nMax = cams[c].n > nMax ? cams[c].n : nMax;
    V.valid = mf->valid, V.maxPts = mf->maxPts, V.dim = mf->dim;
    if (nMax == 0) return CS_OK;
    hipLaunchKernelGGL(k_mf_valid, dim3((nMax + 3) / 4, mf->nCams), dim3(MF_T), 0, s, V);
    CS_CHECK_LAUNCH();
    return CS_OK;
}

// matchSurf of one batch (its job table is on the device)
int mf_match_batch(cs_merge_front* mf, hipStream_t s, int nb, const MfJob* jobs, const MfArgs& A) {
    int n1Max = 0;
    for (int k = 0; k < nb; ++k) n1Max = jobs[k].n1 > n1Max ? jobs[k].n1 : n1Max;
    CS_HIP(hipMemsetAsync(A.colBest, 0xff, (size_t)nb * mf->maxPts * 8, s));
    if (n1Max > 0) {
        hipLaunchKernelGGL(k_mf_match, dim3((n1Max + MF_ROWS - 1) / MF_ROWS, nb), dim3(MF_T), 0, s, A);
        CS_CHECK_LAUNCH();
    }
    hipLaunchKernelGGL(k_mf_collect, dim3(nb), dim3(MF_T), 0, s, A);
    CS_CHECK_LAUNCH();
    return CS_OK;
}

// estimateEMat of one batch behind its matches, counts and point rows
int mf_ransac_batch(cs_merge_front* mf, hipStream_t s, int nb, const MfArgs& A) {
    CS_HIP(hipMemsetAsync(A.best, 0, (size_t)nb * 8, s));
    hipLaunchKernelGGL(k_mf_hyp, dim3((A.nHyp + 3) / 4, nb), dim3(64), 0, s, A);
    CS_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_mf_score, dim3(A.nHyp, nb), dim3(MF_T), 0, s, A);
    CS_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_mf_refit, dim3(nb), dim3(MF_T), 0, s, A);
    CS_CHECK_LAUNCH();
    return CS_OK;
}

int mf_run(const char* who, cs_merge_front* mf, void* hip_stream, const cs_merge_front_cam* cams, int nJobs, const cs_merge_front_job* jobs,
           const MfParams& P, bool ransac) {
    std::vector<MfJob> all;
    int rc = mf_check(who, mf, cams, nJobs, jobs, CS_MERGE_FRONT_MAX_JOBS, true, ransac ? &P : nullptr, all);
    if (rc != CS_OK || nJobs == 0) return rc;
    hipStream_t s = (hipStream_t)hip_stream;
    CS_HIP(hipSetDevice(mf->device));
    if ((rc = mf->stage.begin(s)) != CS_OK || (rc = mf_valid(mf, s, cams)) != CS_OK) return rc;
    const MfArgs A = mf_args(mf, P);
    for (int k0 = 0; k0 < nJobs; k0 += mf->maxJobs) {   // a batch: the work tables are the batch's, the outputs are every job's
        const int nb = nJobs - k0 < mf->maxJobs ? nJobs - k0 : mf->maxJobs;
        if ((rc = mf->stage.upload(s, mf->jobs, all.data() + k0, sizeof(MfJob) * (size_t)nb)) != CS_OK) return rc;
        if ((rc = mf_match_batch(mf, s, nb, all.data() + k0, A)) != CS_OK) return rc;
        if (ransac && (rc = mf_ransac_batch(mf, s, nb, A)) != CS_OK) return rc;
    }
    return CS_OK;
}

}  // namespace

extern "C" int cs_merge_front_run_dev(cs_merge_front* mf, void* hip_stream, const cs_merge_front_cam* cams, int nJobs,
                                      const cs_merge_front_job* jobs, double ratio, double maxDist, int nRansac, double maxEpiErr,
                                      int minInlierNum, unsigned long long seed) {
    const MfParams P = {(float)ratio, (float)maxDist, nRansac, maxEpiErr, minInlierNum, seed};
    return mf_run("cs_merge_front_run_dev", mf, hip_stream, cams, nJobs, jobs, P, true);
}

extern "C" int cs_merge_front_match_dev(cs_merge_front* mf, void* hip_stream, const cs_merge_front_cam* cams, int nJobs,
                                        const cs_merge_front_job* jobs, double ratio, double maxDist) {
    const MfParams P = {(float)ratio, (float)maxDist, 1, 0.0, 0, 0ull};
    return mf_run("cs_merge_front_match_dev", mf, hip_stream, cams, nJobs, jobs, P, false);
}

extern "C" int cs_merge_front_from_matches_dev(cs_merge_front* mf, void* hip_stream, const cs_merge_front_cam* cams, int nJobs,
                                               const cs_merge_front_job* jobs, const int* const* matches, const int* nMatches, int nRansac,
                                               double maxEpiErr, int minInlierNum, unsigned long long seed) {
    const char* who = "cs_merge_front_from_matches_dev";
    const MfParams P = {0.0f, 0.0f, nRansac, maxEpiErr, minInlierNum, seed};
    std::vector<MfJob> all;
    int rc = mf_check(who, mf, cams, nJobs, jobs, mf ? mf->maxJobs : 0, false, &P, all);
    if (rc != CS_OK) return rc;
    if (nJobs > 0 && (!matches || !nMatches)) {
        cs_set_error("%s: null match table", who);
        return CS_ERR_INVALID;
    }
    int nMax = 0;
    for (int k = 0; k < nJobs; ++k) {
        if (nMatches[k] < 0 || nMatches[k] > mf->maxPts || (nMatches[k] > 0 && !matches[k])) {
            cs_set_error("%s: job %d: %d matches (the handle holds %d) or a null list", who, k, nMatches[k], mf->maxPts);
            return CS_ERR_INVALID;
        }
        nMax = nMatches[k] > nMax ? nMatches[k] : nMax;
    }
    if (nJobs == 0) return CS_OK;
    hipStream_t s = (hipStream_t)hip_stream;
    CS_HIP(hipSetDevice(mf->device));
    if ((rc = mf->stage.begin(s)) != CS_OK) return rc;
    const MfArgs A = mf_args(mf, P);
    if ((rc = mf->stage.upload(s, mf->jobs, all.data(), sizeof(MfJob) * (size_t)nJobs)) != CS_OK) return rc;
    if ((rc = mf->stage.upload(s, A.count, nMatches, sizeof(int) * (size_t)nJobs)) != CS_OK) return rc;
    for (int k = 0; k < nJobs; ++k)
        if ((rc = mf->stage.upload(s, A.matches + 2 * (size_t)k * mf->maxPts, matches[k], 8 * (size_t)nMatches[k])) != CS_OK) return rc;
    if (nMax > 0) {
        hipLaunchKernelGGL(k_mf_gather, dim3((nMax + MF_T - 1) / MF_T, nJobs), dim3(MF_T), 0, s, A);
        CS_CHECK_LAUNCH();
    }
    return mf_ransac_batch(mf, s, nJobs, A);
}

extern "C" int cs_merge_front_results(cs_merge_front* mf, void* hip_stream, int nJobs, cs_merge_front_result* h_out) {
    if (!mf || nJobs < 0 || nJobs > CS_MERGE_FRONT_MAX_JOBS || (nJobs > 0 && !h_out)) {
        cs_set_error("cs_merge_front_results: bad arguments");
        return CS_ERR_INVALID;
    }
    CS_HIP(hipSetDevice(mf->device));
    if (nJobs > 0)
        CS_HIP(hipMemcpyAsync(h_out, mf->b.results, sizeof(cs_merge_front_result) * (size_t)nJobs, hipMemcpyDeviceToHost, (hipStream_t)hip_stream));
    CS_HIP(hipStreamSynchronize((hipStream_t)hip_stream));
    return CS_OK;
}

extern "C" int cs_merge_front_buffers_get(const cs_merge_front* mf, cs_merge_front_buffers* out) {
    if (!mf || !out) {
        cs_set_error("cs_merge_front_buffers_get: bad arguments");
        return CS_ERR_INVALID;
    }
    *out = mf->b;
    return CS_OK;
}

extern "C" int cs_merge_front_download(cs_merge_front* mf, void* hip_stream, const void* d_src, void* h_dst, size_t bytes) {
    return cs_arena_download("cs_merge_front_download", mf ? mf->device : 0, mf ? mf->base : nullptr, mf ? mf->bytes : 0, hip_stream, d_src, h_dst,
                             bytes);
}
