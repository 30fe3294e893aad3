// merge_match.hip -- the matcher of a camera-group merge, gfx950: MergeCameraGroup::matchFeaturePointsNCC
// (reference src/app/SL_MergeCameraGroup.cpp:262-307) behind storeFeaturePoints (:179-188); DESIGN.md 3.24.
//
// Per candidate camera pair (a JOB) the host brings the essential matrix and the inlier SURF matches' positions (the seeds); from there:
//   blocks      getScaledNCCBlocks: the 11 x 11 sub-pixel block of EVERY slot from the key frame's small image (ncc.hip's cutter through
//               cs_ncc_get_scaled_blocks_group_dev; k_mm_prep writes the mask `state 0 / 1` and a copy of the positions in which a dead
//               slot's or a non-finite position is 0, so that the cutter never sees a value it cannot turn into a pixel index)
//   candidates  getEpiNccMat as a list (ncc.hip's k_ncc_epi_mat<true>, <= 8 jobs a launch)
//   matches     k_merge_match: the disparity guide, the greedy one-to-one matching and the matches' order, one workgroup per job.
//
// k_merge_match.  Un-vendored LibVisualSLAM, OUR definitions (newpts.hip:15-21), operation for operation:
//   guide    the seed nearest to c1_i in image 1 by squared distance, the first of equals; (i, j) survives iff
//            sqrt(ex^2 + ey^2) <= maxDisp, e = (c2_j - c1_i) - (s2_k - s1_k); a NaN fails; no seeds: no guide.  The nearest seed depends
//            on the row only: found once per row that a candidate names.
//   greedy   the survivors in the total order (score falling, row rising, column rising); a candidate is a match when neither its row nor
//            its column has one.
// There is no cap below pairCap, hence no sort of the list in LDS (k_np_match's 2048 entries).  Built: ROUNDS OF LOCALLY DOMINANT
// CANDIDATES.  Every round each live candidate bids for its row and its column with an atomic maximum of an order-preserving 64-bit image
// of its score; equal bids are settled by an atomic minimum of the column (for a row) and of the row (for a column).  A candidate that holds
// both its row and its column is a match: it is the first live candidate the sequential walk would reach on its row and on its column, so the
// walk accepts it whatever else it accepts before.  Its row's and column's other candidates die; the list is compacted.  The best live candidate
// of all is always such a one, so every round accepts at least one match and a match takes a row: at most N rounds (the loop's bound).  The
// set of matches is the sequential greedy's and nothing depends on the order of the list (maxima, minima and a compare-and-swap on integers).
// The matches are then ranked by the same total order (a count over <= N winners, broadcast lane by lane) and written in that order.
// Why rounds and not a sort: the list holds tens of thousands of candidates of which a few hundred survive as matches; a round is three
// passes of atomics over a list that shrinks fast (tools/mergematch_time.py records the round counts), a global sort is ~log^2 passes over all.
#include <climits>
#include <vector>

#include "cs_common.h"
#include "dev_arena.h"
#include "host33.h"

#pragma clang fp contract(off)

namespace {

constexpr int MM_MAX_CAMS = 16, MM_MAX_N = 32768 /* NP_MAX_N: slot pairs are packed into 16 bits each */, MM_T = 1024, MM_EPI_JOBS = 8;

typedef unsigned long long mm_u64;

struct MmJob {
    const cs_ncc_pair* pairs;
    const int* pairCount;
    const double *xy1, *xy2;   // 2N each: x[N] then y[N]
    const double* seeds;       // [nSeeds][4], device
    int nSeeds, out;           // out: the job's row of the outputs
    int flags;                 // CS_MERGE_MATCH_SKIPPED | CS_MERGE_MATCH_SEEDS_OVERFLOW (k_mm_front_jobs): the job has no candidates
};
struct MmArgs {
    const MmJob* jobs;
    int N, pairCap, maxMatches;
    double maxDisp;
    mm_u64* liveKey;   // [slots][2][pairCap]
    unsigned* liveIJ;  // [slots][2][pairCap]
    mm_u64 *rowBest, *colBest, *winKey;                          // [slots][N]
    int *rowTie, *colTie, *rowMatch, *colMatch, *rowSeed;        // [slots][N]
    unsigned* winIJ;                                             // [slots][N]
    int* matches;      // [CS_MERGE_MATCH_MAX_JOBS][maxMatches][2]
    double* scores;    // [CS_MERGE_MATCH_MAX_JOBS][maxMatches]
    int* counts;       // [CS_MERGE_MATCH_MAX_JOBS][4]
};

// order-preserving image of a binary64 score (no NaN): a < b <=> key(a) < key(b); -0 and +0 share a key (a score of -0 is
// reported as +0: the one place where the output is not the input's bits); every key is > 0
__device__ __forceinline__ mm_u64 mm_key(double s) {
    const mm_u64 b = (mm_u64)__double_as_longlong(s + 0.0);
    return (b >> 63) ? ~b : (b | (1ull << 63));
}
__device__ __forceinline__ double mm_score(mm_u64 k) {
    const mm_u64 b = (k >> 63) ? (k & ~(1ull << 63)) : ~k;
    return __longlong_as_double((long long)b);
}
// the tables are written with atomics (performed in L2) and read back by other waves of the workgroup: read them there as well
template <typename T>
__device__ __forceinline__ T mm_ld(const T* p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
template <typename T>
__device__ __forceinline__ void mm_st(T* p, T v) {
    __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// position of a kept entry behind *counter (LDS), one atomic per wave; called by every lane of the wave
__device__ __forceinline__ int mm_append(bool keep, int* counter) {
    const mm_u64 m = __ballot(keep);
    if (!m) return -1;
    const int lane = threadIdx.x & 63, leader = __ffsll((long long)m) - 1;
    int base = 0;
    if (lane == leader) base = atomicAdd(counter, __popcll(m));
    base = __shfl(base, leader, 64);
    return keep ? base + __popcll(m & ((1ull << lane) - 1)) : -1;
}

__global__ __launch_bounds__(MM_T) void k_merge_match(MmArgs A) {
    const MmJob J = A.jobs[blockIdx.x];
    const int tid = threadIdx.x, N = A.N;
    const size_t jb = blockIdx.x;
    mm_u64* const rowBest = A.rowBest + jb * N;
    mm_u64* const colBest = A.colBest + jb * N;
    mm_u64* const winKey = A.winKey + jb * N;
    unsigned* const winIJ = A.winIJ + jb * N;
    int* const rowTie = A.rowTie + jb * N;
    int* const colTie = A.colTie + jb * N;
    int* const rowMatch = A.rowMatch + jb * N;
    int* const colMatch = A.colMatch + jb * N;
    int* const rowSeed = A.rowSeed + jb * N;
    mm_u64* const key0 = A.liveKey + jb * 2 * A.pairCap;   // list 1 follows list 0 (pointer arithmetic, no indexed array: no scratch)
    unsigned* const ij0 = A.liveIJ + jb * 2 * A.pairCap;
    __shared__ int sCnt[4];            // entries of list 0, of list 1, winners

    const int total = J.flags ? 0 : *J.pairCount;
    const int n = total < 0 ? 0 : (total < A.pairCap ? total : A.pairCap);
    for (int i = tid; i < N; i += MM_T) {
        rowBest[i] = 0, colBest[i] = 0, rowTie[i] = INT_MAX, colTie[i] = INT_MAX, rowMatch[i] = -1, colMatch[i] = -1, rowSeed[i] = -2;
    }
    if (tid < 4) sCnt[tid] = 0;
    __syncthreads();

    // ---- the guide's seed of every row a candidate names: nearest in image 1, the first of equals ----
    if (J.nSeeds > 0) {
        for (int q = tid; q < n; q += MM_T) {
            const int i = J.pairs[q].i;
            if ((unsigned)i < (unsigned)N) mm_st(&rowSeed[i], -1);
        }
        __syncthreads();
        for (int i = tid; i < N; i += MM_T) {
            if (mm_ld(&rowSeed[i]) != -1) continue;
            const double x1 = J.xy1[i], y1 = J.xy1[N + i];
            double best = 1.0e300;
            int bk = 0;
            for (int k = 0; k < J.nSeeds; ++k) {
                const double dx = J.seeds[4 * k] - x1, dy = J.seeds[4 * k + 1] - y1, d2 = dx * dx + dy * dy;
                if (d2 < best) best = d2, bk = k;
            }
            mm_st(&rowSeed[i], bk);
        }
        __syncthreads();
    }

    // ---- the guide; the survivors packed into list 0 ----
    for (int q0 = 0; q0 < n; q0 += MM_T) {
        const int q = q0 + tid;
        bool keep = false;
        int i = 0, j = 0;
        double s = 0;
        if (q < n) {
            const cs_ncc_pair p = J.pairs[q];
            i = p.i, j = p.j, s = p.ncc;
            keep = (unsigned)i < (unsigned)N && (unsigned)j < (unsigned)N && s == s;
            if (keep && J.nSeeds > 0) {
                const double* sd = J.seeds + 4 * mm_ld(&rowSeed[i]);
                const double x1 = J.xy1[i], y1 = J.xy1[N + i];
                const double ex = (J.xy2[j] - x1) - (sd[2] - sd[0]), ey = (J.xy2[N + j] - y1) - (sd[3] - sd[1]);
                keep = sqrt(ex * ex + ey * ey) <= A.maxDisp;
            }
        }
        const int pos = mm_append(keep, &sCnt[0]);
        if (keep) key0[pos] = mm_key(s), ij0[pos] = ((unsigned)i << 16) | (unsigned)j;
    }
    __syncthreads();

    // ---- rounds of locally dominant candidates ----
    int cur = 0, nLive = sCnt[0], rounds = 0;
    while (nLive > 0 && rounds < N) {   // a round accepts at least the best live candidate and a match takes a row: <= N rounds
        const mm_u64* kc = key0 + (size_t)cur * A.pairCap;
        const unsigned* ic = ij0 + (size_t)cur * A.pairCap;
        mm_u64* const kn = key0 + (size_t)(cur ^ 1) * A.pairCap;
        unsigned* const in = ij0 + (size_t)(cur ^ 1) * A.pairCap;
        if (tid == 0) sCnt[cur ^ 1] = 0;
        for (int q = tid; q < nLive; q += MM_T) {
            const mm_u64 k = kc[q];
            const unsigned ij = ic[q];
            atomicMax(&rowBest[ij >> 16], k);
            atomicMax(&colBest[ij & 0xffffu], k);
        }
        __syncthreads();
        for (int q = tid; q < nLive; q += MM_T) {
            const mm_u64 k = kc[q];
            const int i = (int)(ic[q] >> 16), j = (int)(ic[q] & 0xffffu);
            const mm_u64 rb = mm_ld(&rowBest[i]), cb = mm_ld(&colBest[j]);
            if (k == rb) atomicMin(&rowTie[i], j);
            if (k == cb) atomicMin(&colTie[j], i);
        }
        __syncthreads();
        for (int q = tid; q < nLive; q += MM_T) {
            const mm_u64 k = kc[q];
            const int i = (int)(ic[q] >> 16), j = (int)(ic[q] & 0xffffu);
            const mm_u64 rb = mm_ld(&rowBest[i]), cb = mm_ld(&colBest[j]);
            const int rt = mm_ld(&rowTie[i]), ct = mm_ld(&colTie[j]);
            if (k == rb && rt == j && k == cb && ct == i &&
                atomicCAS(&rowMatch[i], -1, j) == -1) {   // (the swap: a pair that the list holds twice is one match)
                mm_st(&colMatch[j], i);
                const int w = atomicAdd(&sCnt[2], 1);      // < N: every winner holds a row of its own
                winKey[w] = k, winIJ[w] = ic[q];
            }
        }
        __syncthreads();
        for (int q0 = 0; q0 < nLive; q0 += MM_T) {
            const int q = q0 + tid;
            bool keep = false;
            mm_u64 k = 0;
            unsigned ij = 0;
            if (q < nLive) {
                k = kc[q], ij = ic[q];
                const int i = (int)(ij >> 16), j = (int)(ij & 0xffffu);
                const int rm = mm_ld(&rowMatch[i]), cm = mm_ld(&colMatch[j]);
                keep = rm < 0 && cm < 0;
                if (keep) {   // a free row / column starts the next round without a bid (every writer writes the same values)
                    mm_st(&rowBest[i], (mm_u64)0), mm_st(&rowTie[i], INT_MAX), mm_st(&colBest[j], (mm_u64)0), mm_st(&colTie[j], INT_MAX);
                }
            }
            const int pos = mm_append(keep, &sCnt[cur ^ 1]);
            if (keep) kn[pos] = k, in[pos] = ij;
        }
        __syncthreads();
        cur ^= 1, nLive = sCnt[cur], ++rounds;
    }

    // ---- acceptance order = the total order: rank every winner among the winners ----
    const int nWin = sCnt[2];
    int2* const outM = (int2*)A.matches + (size_t)J.out * A.maxMatches;
    double* const outS = A.scores + (size_t)J.out * A.maxMatches;
    const int lane = tid & 63;
    for (int w0 = 0; w0 < nWin; w0 += 2 * MM_T) {   // two winners per lane and pass: w0 + tid and w0 + MM_T + tid
        const int wa = w0 + tid, wb = wa + MM_T;
        const bool ha = wa < nWin, hb = wb < nWin;
        const mm_u64 ka = ha ? winKey[wa] : 0, kb = hb ? winKey[wb] : 0;
        const unsigned ia = ha ? winIJ[wa] : 0, ib = hb ? winIJ[wb] : 0;
        int ra = 0, rb = 0;
        for (int v0 = 0; v0 < nWin; v0 += 64) {     // every wave reads every winner: 64 at a time into its lanes ...
            const int v = v0 + lane;
            const mm_u64 ck = v < nWin ? winKey[v] : 0;
            const int ci = v < nWin ? (int)winIJ[v] : 0;
            const int lo = (int)(unsigned)ck, hi = (int)(unsigned)(ck >> 32);
            const int m = nWin - v0 < 64 ? nWin - v0 : 64;
            for (int t = 0; t < m; ++t) {           // ... then lane by lane through v_readlane (t is uniform): no LDS traffic in the count
                const mm_u64 k = ((mm_u64)(unsigned)__builtin_amdgcn_readlane(hi, t) << 32) | (mm_u64)(unsigned)__builtin_amdgcn_readlane(lo, t);
                const unsigned ij = (unsigned)__builtin_amdgcn_readlane(ci, t);
                ra += (k > ka || (k == ka && ij < ia)) ? 1 : 0;
                rb += (k > kb || (k == kb && ij < ib)) ? 1 : 0;
            }
        }
        if (ha && ra < A.maxMatches) {
            outM[ra] = make_int2((int)(ia >> 16), (int)(ia & 0xffffu));
            outS[ra] = mm_score(ka);
        }
        if (hb && rb < A.maxMatches) {
            outM[rb] = make_int2((int)(ib >> 16), (int)(ib & 0xffffu));
            outS[rb] = mm_score(kb);
        }
    }
    if (tid == 0) {
        int* c = A.counts + 4 * (size_t)J.out;
        c[0] = nWin < A.maxMatches ? nWin : A.maxMatches;
        c[1] = J.flags | (total > A.pairCap ? CS_MERGE_MATCH_PAIRS_OVERFLOW : 0) | (nWin > A.maxMatches ? CS_MERGE_MATCH_MATCHES_OVERFLOW : 0);
        c[2] = total, c[3] = rounds;
    }
}

// storeFeaturePoints as a mask, and the positions the cutter and the candidate kernel read
struct MmPrepArgs {
    const double* xy[MM_MAX_CAMS];
    const int* state[MM_MAX_CAMS];
    double* xs;   // [nCams][2N]
    int* valid;   // [nCams][N]
    int N;
};
__global__ __launch_bounds__(256) void k_mm_prep(MmPrepArgs A) {
    const int c = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
    if (i >= A.N) return;
    const int st = A.state[c][i];
    const bool live = st == 0 || st == 1;
    double x = A.xy[c][i], y = A.xy[c][A.N + i];
    const bool ok = live && fabs(x) < 1.0e6 && fabs(y) < 1.0e6;   // a live slot with a non-finite or absurd position takes no part (no pixel index exists for it)
    if (!ok) x = 0, y = 0;
    A.xs[(size_t)c * 2 * A.N + i] = x, A.xs[(size_t)c * 2 * A.N + A.N + i] = y;
    A.valid[(size_t)c * A.N + i] = ok ? 1 : 0;
}

// ---- the jobs of cs_merge_match_run_front_dev: from the front's result records and seed rows, all in device memory ------------------
// A thread per job.  Skipped (surfNum < minSurfNum or no E) or more inliers than seed rows the handle or the front's block holds: the
// flag, no seeds, and an F of NaN -- k_ncc_epi_mat's `epiErr <= epiMax` is then false for every pair, so the job has no candidates.
// Otherwise F = iK1^T E^T iK2 in cs_merge_match_fmat's operation order (this file is compiled with contraction off), and the seed rows
// are read where the front left them.
struct MmFrontArgs {
    const cs_merge_front_result* results;
    const double* seeds;          // [..][seedRows][4]
    const int2* cams;             // [nJobs] {iCam, jCam}
    const double* iK;             // [nCams][9]
    cs_merge_match_front_job* rec;   // [CS_MERGE_MATCH_MAX_JOBS]
    MmJob* jobs;                  // [CS_MERGE_MATCH_MAX_JOBS]
    const cs_ncc_pair* pairs;
    const int* pairCount;
    const double* xs;
    int nJobs, seedRows, minSurfNum, maxSeeds, maxJobs, pairCap, N;
};
__global__ __launch_bounds__(256) void k_mm_front_jobs(MmFrontArgs A) {
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k >= A.nJobs) return;
    const cs_merge_front_result r = A.results[k];
    const int2 cam = A.cams[k];
    int flags = 0;
    if (r.surfNum < A.minSurfNum || !r.ematOk)
        flags = CS_MERGE_MATCH_SKIPPED;
    else if (r.inlierNum > A.maxSeeds || r.inlierNum > A.seedRows)
        flags = CS_MERGE_MATCH_SEEDS_OVERFLOW;
    double F[9];
    if (flags) {
        for (int q = 0; q < 9; ++q) F[q] = __longlong_as_double(0x7ff8000000000000ll);
    } else {
        const double *iK1 = A.iK + 9 * cam.x, *iK2 = A.iK + 9 * cam.y;
        double T[9];
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 3; ++j) {
                double t = 0;
                for (int q = 0; q < 3; ++q) t += iK1[3 * q + i] * r.E[3 * j + q];
                T[3 * i + j] = t;
            }
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 3; ++j) F[3 * i + j] = (T[3 * i] * iK2[j] + T[3 * i + 1] * iK2[3 + j]) + T[3 * i + 2] * iK2[6 + j];
    }
    const int nSeeds = flags || r.inlierNum < 0 ? 0 : r.inlierNum, slot = k % A.maxJobs;
    cs_merge_match_front_job& R = A.rec[k];
    for (int q = 0; q < 9; ++q) R.F[q] = F[q];
    R.nSeeds = nSeeds, R.flags = flags;
    MmJob J;
    J.pairs = A.pairs + (size_t)slot * A.pairCap, J.pairCount = A.pairCount + slot;
    J.xy1 = A.xs + (size_t)cam.x * 2 * A.N, J.xy2 = A.xs + (size_t)cam.y * 2 * A.N;
    J.seeds = A.seeds + (size_t)k * A.seedRows * 4, J.nSeeds = nSeeds, J.out = k, J.flags = flags;
    A.jobs[k] = J;
}

}  // namespace

struct cs_merge_match {
    int device, nCams, N, maxJobs, maxSeeds, pairCap, maxMatches;
    char* base;
    size_t bytes;
    cs_merge_match_buffers b;
    double* xs;
    double* seeds;   // [maxJobs][maxSeeds][4]
    MmJob* jobs;     // [maxJobs]
    MmJob* frontJobs;                      // [CS_MERGE_MATCH_MAX_JOBS]: k_mm_front_jobs' table
    cs_merge_match_front_job* frontRec;    // [CS_MERGE_MATCH_MAX_JOBS]
    int2* frontCams;                       // [CS_MERGE_MATCH_MAX_JOBS]
    double* iK;                            // [nCams][9]
    MmArgs args;     // the tables (jobs / maxDisp are set per launch)
    CsStage stage;
};

// the device block: per camera slot, the candidate lists, the matcher's work tables per batch slot, per job
static void mm_layout(cs_merge_match* mm, CsArena& ar) {
    const size_t nS = (size_t)mm->nCams * mm->N, nJ = mm->maxJobs, nL = nJ * 2 * (size_t)mm->pairCap, nT = nJ * mm->N, nO = CS_MERGE_MATCH_MAX_JOBS;
    cs_merge_match_buffers& B = mm->b;
    MmArgs& A = mm->args;
    ar.take(B.blocks, nS * 128), ar.take(B.abc, nS * 4), ar.take(B.valid, nS), ar.take(mm->xs, nS * 2);
    ar.take(B.pairs, nJ * mm->pairCap), ar.take(B.pairCount, nJ);
    ar.take(A.liveKey, nL), ar.take(A.liveIJ, nL);
    ar.take(A.rowBest, nT), ar.take(A.colBest, nT), ar.take(A.winKey, nT);
    ar.take(A.rowTie, nT), ar.take(A.colTie, nT), ar.take(A.rowMatch, nT), ar.take(A.colMatch, nT), ar.take(A.rowSeed, nT), ar.take(A.winIJ, nT);
    ar.take(mm->seeds, nJ * (size_t)(mm->maxSeeds > 0 ? mm->maxSeeds : 1) * 4), ar.take(mm->jobs, nJ);
    ar.take(mm->frontJobs, nO), ar.take(mm->frontRec, nO), ar.take(mm->frontCams, nO), ar.take(mm->iK, (size_t)mm->nCams * 9);
    ar.take(A.matches, nO * mm->maxMatches * 2), ar.take(A.scores, nO * mm->maxMatches), ar.take(A.counts, nO * 4);
}

extern "C" int cs_merge_match_fmat(const double K1[9], const double K2[9], const double E[9], double F[9]) {
    double iK1[9], iK2[9], T[9];
    if (!K1 || !K2 || !E || !F || !cs_host_inv33(K1, iK1) || !cs_host_inv33(K2, iK2)) {
        cs_set_error("cs_merge_match_fmat: null argument or singular K");
        return CS_ERR_INVALID;
    }
    // mat33Trans(E, Et); getFMat(iK2, iK1, Et, F): F = iK1^T Et iK2 (getFMat(a, b, E, F) = b^T E a)
    for (int i = 0; i < 3; ++i)   // T = iK1^T Et, accumulated from 0 (matATB)
        for (int j = 0; j < 3; ++j) {
            double t = 0;
            for (int k = 0; k < 3; ++k) t += iK1[3 * k + i] * E[3 * j + k];
            T[3 * i + j] = t;
        }
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) F[3 * i + j] = (T[3 * i] * iK2[j] + T[3 * i + 1] * iK2[3 + j]) + T[3 * i + 2] * iK2[6 + j];
    return CS_OK;
}

extern "C" cs_merge_match* cs_merge_match_create(int device, int nCams, int N, int maxJobs, int maxSeeds, int pairCap, int maxMatches) {
    if (nCams < 1 || nCams > MM_MAX_CAMS || N < 1 || N > MM_MAX_N || maxJobs < 1 || maxJobs > CS_MERGE_MATCH_MAX_JOBS || maxSeeds < 0 ||
        pairCap < 1 || maxMatches < 1 || maxMatches > (1 << 24) || pairCap > (1 << 28)) {
        cs_set_error("cs_merge_match_create: bad argument (nCams %d of 1..%d, N %d of 1..%d, maxJobs %d of 1..%d, maxSeeds %d, pairCap %d, maxMatches %d)",
                     nCams, MM_MAX_CAMS, N, MM_MAX_N, maxJobs, CS_MERGE_MATCH_MAX_JOBS, maxSeeds, pairCap, maxMatches);
        return nullptr;
    }
    cs_merge_match* mm = new cs_merge_match();
    mm->device = device, mm->nCams = nCams, mm->N = N, mm->maxJobs = maxJobs, mm->maxSeeds = maxSeeds, mm->pairCap = pairCap, mm->maxMatches = maxMatches;
    cs_merge_match_buffers& B = mm->b;
    MmArgs& A = mm->args;
    memset(&A, 0, sizeof(A));
    if (!cs_arena_alloc(device, mm->base, mm->bytes, [mm](CsArena& ar) { mm_layout(mm, ar); })) {
        cs_set_error("cs_merge_match_create: %zu bytes of device memory: %s", mm->bytes, hipGetErrorString(hipGetLastError()));
        delete mm;
        return nullptr;
    }
    A.N = N, A.pairCap = pairCap, A.maxMatches = maxMatches;
    B.matches = A.matches, B.scores = A.scores, B.counts = A.counts;
    B.nCams = nCams, B.N = N, B.maxJobs = maxJobs, B.maxSeeds = maxSeeds, B.pairCap = pairCap, B.maxMatches = maxMatches;
    return mm;
}

extern "C" void cs_merge_match_destroy(cs_merge_match* mm) {
    if (!mm) return;
    if (mm->base) {
        (void)hipSetDevice(mm->device);
        mm->stage.drain();   // (an upload of the last call may still read its staging copy)
        (void)hipFree(mm->base);
    }
    delete mm;
}

// the jobs' table and seeds of one batch to the device, then the matcher: nb workgroups
static int mm_launch(cs_merge_match* mm, hipStream_t s, int nb, const MmJob* jobs, const int* nSeeds, const double* const* seeds, double maxDisp) {
    const size_t seedBytes = (size_t)(mm->maxSeeds > 0 ? mm->maxSeeds : 1) * 32;
    int rc = mm->stage.upload(s, mm->jobs, jobs, sizeof(MmJob) * (size_t)nb);
    if (rc != CS_OK) return rc;
    size_t need = 0;
    for (int k = 0; k < nb; ++k)
        if (nSeeds[k] > 0) need = (size_t)(k + 1) * seedBytes;
    if (need) {
        char* h = mm->stage.block(need);
        memset(h, 0, need);
        for (int k = 0; k < nb; ++k)
            if (nSeeds[k] > 0) memcpy(h + k * seedBytes, seeds[k], (size_t)nSeeds[k] * 32);
        CS_HIP(hipMemcpyAsync(mm->seeds, h, need, hipMemcpyHostToDevice, s));
    }
    MmArgs A = mm->args;
    A.jobs = mm->jobs, A.maxDisp = maxDisp;
    hipLaunchKernelGGL(k_merge_match, dim3(nb), dim3(MM_T), 0, s, A);
    CS_CHECK_LAUNCH();
    return CS_OK;
}

extern "C" int cs_merge_match_from_pairs_dev(cs_merge_match* mm, void* hip_stream, int nJobs, const cs_ncc_pair* const* d_pairs,
                                             const int* const* d_pairCount, const double* const* d_xy1, const double* const* d_xy2,
                                             const int* nSeeds, const double* const* seeds, double maxDisp) {
    const char* who = "cs_merge_match_from_pairs_dev";
    if (!mm || nJobs < 0 || (nJobs > 0 && (!d_pairs || !d_pairCount || !d_xy1 || !d_xy2)) || nJobs > mm->maxJobs) {
        cs_set_error("%s: bad arguments (%d jobs, the handle holds %d)", who, nJobs, mm ? mm->maxJobs : 0);
        return CS_ERR_INVALID;
    }
    std::vector<MmJob> jobs((size_t)nJobs);
    std::vector<int> ns((size_t)nJobs, 0);
    const size_t seedDoubles = (size_t)(mm->maxSeeds > 0 ? mm->maxSeeds : 1) * 4;
    for (int k = 0; k < nJobs; ++k) {
        ns[k] = nSeeds ? nSeeds[k] : 0;
        if (!d_pairs[k] || !d_pairCount[k] || !d_xy1[k] || !d_xy2[k] || ns[k] < 0 || ns[k] > mm->maxSeeds || (ns[k] > 0 && (!seeds || !seeds[k]))) {
            cs_set_error("%s: job %d: null table or %d seeds (the handle holds %d)", who, k, ns[k], mm->maxSeeds);
            return CS_ERR_INVALID;
        }
        jobs[k] = MmJob{d_pairs[k], d_pairCount[k], d_xy1[k], d_xy2[k], mm->seeds + k * seedDoubles, ns[k], k};
    }
    if (nJobs == 0) return CS_OK;
    hipStream_t s = (hipStream_t)hip_stream;
    CS_HIP(hipSetDevice(mm->device));
    int rc = mm->stage.begin(s);
    if (rc != CS_OK) return rc;
    return mm_launch(mm, s, nJobs, jobs.data(), ns.data(), seeds, maxDisp);
}

// the cameras of a call: refused when a table is missing, else the cutter's / candidate kernel's view of them
static int mm_cams(cs_merge_match* mm, const char* who, const cs_merge_match_cam* cams, cs_ncc_cam* nc) {
    const int nC = mm->nCams, N = mm->N;
    memset(nc, 0, sizeof(cs_ncc_cam) * MM_MAX_CAMS);
    for (int c = 0; c < nC; ++c) {
        if (!cams[c].xy || !cams[c].state || !cams[c].K || !cams[c].imgSmall || !(cams[c].imgScale > 0)) {
            cs_set_error("%s: camera %d: null xy / state / K / imgSmall, or imgScale %g", who, c, cams[c].imgScale);
            return CS_ERR_INVALID;
        }
        nc[c].img = cams[c].imgSmall, nc[c].x = mm->xs + (size_t)c * 2 * N, nc[c].y = nc[c].x + N;
        nc[c].blocks = (unsigned char*)mm->b.blocks + (size_t)c * N * 128, nc[c].abc = (double*)mm->b.abc + (size_t)c * N * 4;
        nc[c].valid = (int*)mm->b.valid + (size_t)c * N;
    }
    return CS_OK;
}

// the mask and the positions, then every slot's block
static int mm_blocks(cs_merge_match* mm, void* hip_stream, const cs_merge_match_cam* cams, const cs_ncc_cam* nc, int Ws, int Hs) {
    const int nC = mm->nCams, N = mm->N;
    hipStream_t s = (hipStream_t)hip_stream;
    MmPrepArgs P;
    memset(&P, 0, sizeof(P));
    for (int c = 0; c < nC; ++c) P.xy[c] = cams[c].xy, P.state[c] = cams[c].state;
    P.xs = mm->xs, P.valid = (int*)mm->b.valid, P.N = N;
    hipLaunchKernelGGL(k_mm_prep, dim3((N + 255) / 256, nC), dim3(256), 0, s, P);
    CS_CHECK_LAUNCH();
    bool cut[MM_MAX_CAMS] = {false};
    for (int c = 0; c < nC; ++c) {   // the cutter takes one scale a launch: one launch per DISTINCT imgScale (KeyPose::imgScale is per camera)
        if (cut[c]) continue;
        cs_ncc_cam sub[MM_MAX_CAMS];
        int nSub = 0;
        for (int d = c; d < nC; ++d)
            if (!cut[d] && cams[d].imgScale == cams[c].imgScale) sub[nSub++] = nc[d], cut[d] = true;
        const int rc = cs_ncc_get_scaled_blocks_group_dev(mm->device, hip_stream, nSub, sub, Ws, Hs, N, cams[c].imgScale);
        if (rc != CS_OK) return rc;
    }
    return CS_OK;
}

extern "C" int cs_merge_match_run_dev(cs_merge_match* mm, void* hip_stream, const cs_merge_match_cam* cams, int Ws, int Hs, int nJobs,
                                      const cs_merge_match_job* jobs, double epiMax, double nccMin, double maxDisp) {
    const char* who = "cs_merge_match_run_dev";
    if (!mm || !cams || Ws < 1 || Hs < 1 || nJobs < 0 || nJobs > CS_MERGE_MATCH_MAX_JOBS || (nJobs > 0 && !jobs)) {
        cs_set_error("%s: bad arguments (%d jobs of at most %d, small image %d x %d)", who, nJobs, CS_MERGE_MATCH_MAX_JOBS, Ws, Hs);
        return CS_ERR_INVALID;
    }
    const int nC = mm->nCams, N = mm->N;
    cs_ncc_cam nc[MM_MAX_CAMS];
    if (mm_cams(mm, who, cams, nc) != CS_OK) return CS_ERR_INVALID;
    std::vector<cs_ncc_pair_job> pj((size_t)nJobs);
    for (int k = 0; k < nJobs; ++k) {
        const cs_merge_match_job& q = jobs[k];
        if (q.iCam < 0 || q.iCam >= nC || q.jCam < 0 || q.jCam >= nC || q.iCam == q.jCam || q.nSeeds < 0 || q.nSeeds > mm->maxSeeds ||
            (q.nSeeds > 0 && !q.seeds)) {
            cs_set_error("%s: job %d: cameras %d / %d of %d, %d seeds (the handle holds %d)", who, k, q.iCam, q.jCam, nC, q.nSeeds, mm->maxSeeds);
            return CS_ERR_INVALID;
        }
        memset(&pj[k], 0, sizeof(pj[k]));
        if (cs_merge_match_fmat(cams[q.iCam].K, cams[q.jCam].K, q.E, pj[k].F) != CS_OK) return CS_ERR_INVALID;
        const int slot = k % mm->maxJobs;
        pj[k].camA = q.iCam, pj[k].camB = q.jCam;
        pj[k].pairs = (cs_ncc_pair*)mm->b.pairs + (size_t)slot * mm->pairCap, pj[k].count = (int*)mm->b.pairCount + slot;
    }
    hipStream_t s = (hipStream_t)hip_stream;
    CS_HIP(hipSetDevice(mm->device));
    int rc = mm->stage.begin(s);
    if (rc != CS_OK) return rc;
    rc = mm_blocks(mm, hip_stream, cams, nc, Ws, Hs);
    if (rc != CS_OK) return rc;
    const size_t seedDoubles = (size_t)(mm->maxSeeds > 0 ? mm->maxSeeds : 1) * 4;
    for (int k0 = 0; k0 < nJobs; k0 += mm->maxJobs) {   // a batch: its candidate lists, then its matcher
        const int nb = nJobs - k0 < mm->maxJobs ? nJobs - k0 : mm->maxJobs;
        for (int e0 = 0; e0 < nb; e0 += MM_EPI_JOBS) {
            const int ne = nb - e0 < MM_EPI_JOBS ? nb - e0 : MM_EPI_JOBS;
            rc = cs_ncc_epi_pairs_group_dev(mm->device, hip_stream, nC, nc, N, ne, pj.data() + k0 + e0, epiMax, nccMin, mm->pairCap);
            if (rc != CS_OK) return rc;
        }
        std::vector<MmJob> mj((size_t)nb);
        std::vector<int> ns((size_t)nb);
        std::vector<const double*> sp((size_t)nb);
        for (int k = 0; k < nb; ++k) {
            const cs_merge_match_job& q = jobs[k0 + k];
            mj[k] = MmJob{pj[k0 + k].pairs, pj[k0 + k].count, nc[q.iCam].x, nc[q.jCam].x, mm->seeds + k * seedDoubles, q.nSeeds, k0 + k};
            ns[k] = q.nSeeds, sp[k] = q.seeds;
        }
        rc = mm_launch(mm, s, nb, mj.data(), ns.data(), sp.data(), maxDisp);
        if (rc != CS_OK) return rc;
    }
    return CS_OK;
}

extern "C" int cs_merge_match_run_front_dev(cs_merge_match* mm, void* hip_stream, const cs_merge_match_cam* cams, int Ws, int Hs, int nJobs,
                                            const cs_merge_front_job* pairs, const cs_merge_front_result* d_results, const double* d_seeds,
                                            int seedRowsPerJob, int minSurfNum, double epiMax, double nccMin, double maxDisp) {
    const char* who = "cs_merge_match_run_front_dev";
    if (!mm || !cams || Ws < 1 || Hs < 1 || nJobs < 0 || nJobs > CS_MERGE_MATCH_MAX_JOBS ||
        (nJobs > 0 && (!pairs || !d_results || !d_seeds || seedRowsPerJob < 1))) {
        cs_set_error("%s: bad arguments (%d jobs of at most %d, small image %d x %d, %d seed rows per job)", who, nJobs, CS_MERGE_MATCH_MAX_JOBS, Ws,
                     Hs, seedRowsPerJob);
        return CS_ERR_INVALID;
    }
    const int nC = mm->nCams, N = mm->N;
    cs_ncc_cam nc[MM_MAX_CAMS];
    if (mm_cams(mm, who, cams, nc) != CS_OK) return CS_ERR_INVALID;
    std::vector<double> iK((size_t)nC * 9, 0.0);   // of the cameras a job names: host-computed, as cs_merge_match_fmat inverts them
    std::vector<char> have((size_t)nC, 0);
    std::vector<int2> jc((size_t)nJobs);
    std::vector<cs_ncc_pair_job> pj((size_t)nJobs);
    for (int k = 0; k < nJobs; ++k) {
        const int a = pairs[k].iCam, b = pairs[k].jCam;
        if (a < 0 || a >= nC || b < 0 || b >= nC || a == b) {
            cs_set_error("%s: job %d: cameras %d / %d of %d", who, k, a, b, nC);
            return CS_ERR_INVALID;
        }
        for (int c : {a, b})
            if (!have[c]) {
                if (!cs_host_inv33(cams[c].K, &iK[9 * (size_t)c])) {
                    cs_set_error("%s: job %d: singular K of camera %d", who, k, c);
                    return CS_ERR_INVALID;
                }
                have[c] = 1;
            }
        jc[k] = make_int2(a, b);
        const int slot = k % mm->maxJobs;
        memset(&pj[k], 0, sizeof(pj[k]));
        pj[k].camA = a, pj[k].camB = b, pj[k].dF = mm->frontRec[k].F;   // (an address: the record is in device memory)
        pj[k].pairs = (cs_ncc_pair*)mm->b.pairs + (size_t)slot * mm->pairCap, pj[k].count = (int*)mm->b.pairCount + slot;
    }
    if (nJobs == 0) return CS_OK;
    hipStream_t s = (hipStream_t)hip_stream;
    CS_HIP(hipSetDevice(mm->device));
    int rc = mm->stage.begin(s);
    if (rc != CS_OK) return rc;
    if ((rc = mm->stage.upload(s, mm->iK, iK.data(), sizeof(double) * iK.size())) != CS_OK) return rc;
    if ((rc = mm->stage.upload(s, mm->frontCams, jc.data(), sizeof(int2) * jc.size())) != CS_OK) return rc;
    MmFrontArgs FA;
    FA.results = d_results, FA.seeds = d_seeds, FA.cams = mm->frontCams, FA.iK = mm->iK, FA.rec = mm->frontRec, FA.jobs = mm->frontJobs;
    FA.pairs = (const cs_ncc_pair*)mm->b.pairs, FA.pairCount = (const int*)mm->b.pairCount, FA.xs = mm->xs;
    FA.nJobs = nJobs, FA.seedRows = seedRowsPerJob, FA.minSurfNum = minSurfNum, FA.maxSeeds = mm->maxSeeds, FA.maxJobs = mm->maxJobs;
    FA.pairCap = mm->pairCap, FA.N = N;
    hipLaunchKernelGGL(k_mm_front_jobs, dim3((nJobs + 255) / 256), dim3(256), 0, s, FA);
    CS_CHECK_LAUNCH();
    rc = mm_blocks(mm, hip_stream, cams, nc, Ws, Hs);
    if (rc != CS_OK) return rc;
    for (int k0 = 0; k0 < nJobs; k0 += mm->maxJobs) {   // a batch: its candidate lists, then its matcher on the device-filled table
        const int nb = nJobs - k0 < mm->maxJobs ? nJobs - k0 : mm->maxJobs;
        for (int e0 = 0; e0 < nb; e0 += MM_EPI_JOBS) {
            const int ne = nb - e0 < MM_EPI_JOBS ? nb - e0 : MM_EPI_JOBS;
            rc = cs_ncc_epi_pairs_group_dev(mm->device, hip_stream, nC, nc, N, ne, pj.data() + k0 + e0, epiMax, nccMin, mm->pairCap);
            if (rc != CS_OK) return rc;
        }
        MmArgs A = mm->args;
        A.jobs = mm->frontJobs + k0, A.maxDisp = maxDisp;
        hipLaunchKernelGGL(k_merge_match, dim3(nb), dim3(MM_T), 0, s, A);
        CS_CHECK_LAUNCH();
    }
    return CS_OK;
}

extern "C" int cs_merge_match_front_jobs(cs_merge_match* mm, void* hip_stream, int nJobs, cs_merge_match_front_job* h_out) {
    if (!mm || nJobs < 0 || nJobs > CS_MERGE_MATCH_MAX_JOBS || (nJobs > 0 && !h_out)) {
        cs_set_error("cs_merge_match_front_jobs: bad arguments");
        return CS_ERR_INVALID;
    }
    CS_HIP(hipSetDevice(mm->device));
    if (nJobs > 0)
        CS_HIP(hipMemcpyAsync(h_out, mm->frontRec, sizeof(cs_merge_match_front_job) * (size_t)nJobs, hipMemcpyDeviceToHost, (hipStream_t)hip_stream));
    CS_HIP(hipStreamSynchronize((hipStream_t)hip_stream));
    return CS_OK;
}

extern "C" int cs_merge_match_counts(cs_merge_match* mm, void* hip_stream, int nJobs, cs_merge_match_count* h_out) {
    if (!mm || nJobs < 0 || nJobs > CS_MERGE_MATCH_MAX_JOBS || (nJobs > 0 && !h_out)) {
        cs_set_error("cs_merge_match_counts: bad arguments");
        return CS_ERR_INVALID;
    }
    CS_HIP(hipSetDevice(mm->device));
    if (nJobs > 0) CS_HIP(hipMemcpyAsync(h_out, mm->b.counts, sizeof(cs_merge_match_count) * (size_t)nJobs, hipMemcpyDeviceToHost, (hipStream_t)hip_stream));
    CS_HIP(hipStreamSynchronize((hipStream_t)hip_stream));
    return CS_OK;
}

extern "C" int cs_merge_match_buffers_get(const cs_merge_match* mm, cs_merge_match_buffers* out) {
    if (!mm || !out) {
        cs_set_error("cs_merge_match_buffers_get: bad arguments");
        return CS_ERR_INVALID;
    }
    *out = mm->b;
    return CS_OK;
}

extern "C" int cs_merge_match_download(cs_merge_match* mm, void* hip_stream, const void* d_src, void* h_dst, size_t bytes) {
    return cs_arena_download("cs_merge_match_download", mm ? mm->device : 0, mm ? mm->base : nullptr, mm ? mm->bytes : 0, hip_stream, d_src, h_dst,
                             bytes);
}
