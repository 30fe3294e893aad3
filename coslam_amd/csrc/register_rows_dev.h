// register_rows_dev.h -- the per-row bodies of the registration's second visits, shared by the wide kernels that run one step per launch
// (register.hip: k_register_search, k_revisit_decide) and the one-workgroup launch that plays all rounds of a frame (poseupdate.hip:
// k_revisit_rounds).  Same code in both, so the same bits: a (point, camera) pair of the search is set up and finished by rg_pair_begin /
// rg_pair_finish whoever scans the feature list between them (the nearest feature is the lexicographic minimum on (distance, slot), however
// the list is split), and a round's walks are rv_decide_rows whatever launch they run in.
#pragma once

#include "cs_common.h"

#include <cfloat>

#pragma clang fp contract(off)

namespace {

constexpr int RG_MAX_CAMS = 16;

struct Proj {
    double u, v, w;
    double KR[9];
};

__device__ __forceinline__ void projection_cov(const Proj& q, const double* __restrict__ cov, double sigma, double var[4]) {
    const double ww = q.w * q.w;
    double J[6], JC[6];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        J[j] = (q.KR[j] * q.w - q.u * q.KR[6 + j]) / ww;
        J[3 + j] = (q.KR[3 + j] * q.w - q.v * q.KR[6 + j]) / ww;
    }
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) JC[3 * i + j] = (J[3 * i] * cov[j] + J[3 * i + 1] * cov[3 + j]) + J[3 * i + 2] * cov[6 + j];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const double s = (JC[3 * i] * J[3 * j] + JC[3 * i + 1] * J[3 * j + 1]) + JC[3 * i + 2] * J[3 * j + 2];
            var[2 * i + j] = (i == j) ? s + sigma * sigma : s;
        }
}

__device__ __forceinline__ void mat22_inv(const double A[4], double iA[4]) {
    const double det = A[0] * A[3] - A[1] * A[2];
    iA[0] = A[3] / det;
    iA[1] = -A[1] / det;
    iA[2] = -A[2] / det;
    iA[3] = A[0] / det;
}

__device__ __forceinline__ double maha_dist2(double mx, double my, double bx, double by, const double ivar[4]) {
    const double dx = mx - bx, dy = my - by;
    return dx * (ivar[0] * dx + ivar[1] * dy) + dy * (ivar[2] * dx + ivar[3] * dy);
}

// ---- one (point, camera) pair of the search: SL_CoSLAM.cpp:737-753 in front of the scan, :757-759 and staticCheckMergability's own term
// (:716-725) behind it.  rg_pair_begin: true when the feature list is to be scanned (m0, m1, ivar set); else outSlot says why not (-2 behind
// the camera, -3 outside the image) -- or stays -1: a feature of this frame is attached there already.
__device__ __forceinline__ bool rg_pair_begin(const cs_register_pass& Q, const cs_register_cam& C, size_t o, int p, int W, int H, Proj& q,
                                              double& m0, double& m1, double var[4], double ivar[4], int& outSlot) {
    if (Q.pointFeat[o] >= 0) return false;  // SL_CoSLAM.cpp:737-738: no feature of this frame attached in this camera yet
    const double *K = C.K, *R = C.R, *t = C.t, *M = Q.M + 3 * (size_t)p;
    const double X = ((R[0] * M[0] + R[1] * M[1]) + R[2] * M[2]) + t[0];
    const double Y = ((R[3] * M[0] + R[4] * M[1]) + R[5] * M[2]) + t[1];
    const double Z = ((R[6] * M[0] + R[7] * M[1]) + R[8] * M[2]) + t[2];
    if (Z < 0.0) {  // :740-742 isAtCameraBack
        outSlot = -2;
        return false;
    }
    q.u = (K[0] * X + K[1] * Y) + K[2] * Z;
    q.v = (K[3] * X + K[4] * Y) + K[5] * Z;
    q.w = (K[6] * X + K[7] * Y) + K[8] * Z;
    m0 = q.u / q.w;  // :744-745 project
    m1 = q.v / q.w;
    if (m0 < 0 || m0 >= (double)W || m1 < 0 || m1 >= (double)H) {  // :746-748
        outSlot = -3;
        return false;
    }
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) q.KR[3 * i + j] = (K[3 * i] * R[j] + K[3 * i + 1] * R[3 + j]) + K[3 * i + 2] * R[6 + j];
    projection_cov(q, Q.cov + 9 * (size_t)p, Q.sigmaSearch, var);  // :750-753
    mat22_inv(var, ivar);                                          // SL_SingleSLAM.cpp:1148-1149
    // (the certainly dynamic points of a pass that serves both registrations: their own scale, SL_CoSLAM.cpp:973)
    const bool dynPt = Q.mapFlags && (Q.mapFlags[p] & (CS_MAP_DYNAMIC | CS_MAP_FALSE | CS_MAP_UNCERTAIN)) == CS_MAP_DYNAMIC;
    const double sc = 1 / (dynPt ? Q.maxDistDynamic : Q.maxDist);
#pragma unroll
    for (int k = 0; k < 4; ++k) ivar[k] = ivar[k] * sc;
    return true;
}
// behind the scan: (dMin, iMin) = the lexicographic minimum on (distance, slot) over the list (iMin 0x7fffffff: no feature in this frame)
__device__ __forceinline__ void rg_pair_finish(const cs_register_pass& Q, const cs_register_cam& C, int p, int N, const Proj& q, double m0,
                                               double m1, double dMin, int iMin, int& outSlot, int& outFlags, double& outDist) {
    if (iMin == 0x7fffffff) {
        outSlot = -4;
        return;
    }
    outSlot = iMin;
    outDist = dMin;
    if (C.slot2map[iMin] < 0) outFlags |= 1;               // :759 pFeat->mpt == 0
    if (C.isDynamic ? C.isDynamic[iMin] != 0 : (C.isStatic && C.isStatic[iMin] == 0)) outFlags |= 2;  // :758 pFeat->type
    double v2[4], iv[4];                                   // staticCheckMergability, the candidate itself (:716-725)
    projection_cov(q, Q.cov + 9 * (size_t)p, Q.sigmaMerge, v2);
    mat22_inv(v2, iv);
    if (!(maha_dist2(m0, m1, C.xy[iMin], C.xy[N + iMin], iv) > 1.0)) outFlags |= 4;
}
__device__ __forceinline__ void rg_pair_store(const cs_register_pass& Q, size_t o, int outSlot, int outFlags, double outDist, double m0, double m1,
                                              const double var[4]) {
    Q.slot[o] = outSlot;
    Q.flags[o] = outFlags;
    Q.dist[o] = outDist;
    Q.m[2 * o] = m0;
    Q.m[2 * o + 1] = m1;
#pragma unroll
    for (int k = 0; k < 4; ++k) Q.var[4 * o + k] = var[k];
}
// the scan by ONE wave (k_revisit_rounds: a wave per pair of a short list): lane l takes slots l, l + 64, ... with a strict <, then the lanes'
// minima are merged on (distance, slot) -- the serial loop's "strict <, first wins", as k_register_search's staged scan.  A slot that is not
// in this frame's list is skipped (k_register_search stages it as NaN, which never compares less).  Every lane returns the minimum.
__device__ __forceinline__ void rg_pair_scan_wave(const cs_register_cam& C, int N, int lane, double m0, double m1, const double ivar[4],
                                                  double& dMin, int& iMin) {
    dMin = DBL_MAX, iMin = 0x7fffffff;
    const double* __restrict__ xs = C.xy;
    const double* __restrict__ ys = C.xy + N;
    const int* __restrict__ st = C.state;
    for (int i = lane; i < N; i += 64) {
        const int s = st[i];
        if (s == 0 || s == 1) {
            const double d = maha_dist2(m0, m1, xs[i], ys[i], ivar);
            if (d < dMin) dMin = d, iMin = i;
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const double d2 = __shfl_xor(dMin, off, 64);
        const int i2 = __shfl_xor(iMin, off, 64);
        if (d2 < dMin || (d2 == dMin && i2 < iMin)) dMin = d2, iMin = i2;
    }
}

// ---- the walks' codes and owners (cs_register_decide_*; the second visits' rounds below)
constexpr int RD_MAX_CAMS = 16;
// code of (point, camera): -1 the walk passes the camera by; else the candidate feature camera * N + slot in the low bits and
constexpr int RD_INIT_MAPPED = 1 << 29, RD_CAN_MERGE = 1 << 28, RD_FEAT = (1 << 28) - 1;
constexpr int RD_INF = 0x7fffffff;
__device__ __forceinline__ int rd_ld(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void rd_st(int* p, int v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void rd_st8(unsigned char* p, unsigned char v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
// the decision's scratch (cs_register_decide_scratch_bytes), in ints: head (the self-settling launch's ticket and list count, 0 between
// calls) | code [nCams][P] | base [P] | owner x 3 [nCams * N] | the decision's own rest.  The second visits' rounds borrow the owner arrays.
constexpr int RD_SCRATCH_HEAD = 4;
inline int* rd_scratch_owners(void* scratch, int nCams, int P) { return (int*)scratch + RD_SCRATCH_HEAD + (size_t)nCams * P + P; }

// ---- one round of the SECOND VISITS (register.hip: the rounds' account): the listed points' walks, their Jacobi sweeps among themselves,
// the attach, the next round's list and the conflict count.  ONE workgroup of at least cap threads, a thread per listed row; the caller
// leaves before it on an empty list.
struct RvArgs {
    int nCams, N, P, cap, mapBase, kinds;
    const int* list;                 // [cap]: the points visited again (k_revisit_list)
    const int* nextLoop;             // [P]
    int* visitLoop;                  // [P]
    const int* slot;                 // the search's tables over the listed rows, [P][nCams]
    const int* flags;
    const unsigned char* mergeable;
    const unsigned char* mapFlags;
    int* pointFeat;
    int* slot2map[RD_MAX_CAMS];
    unsigned char* attached;         // [P][nCams]: set where this round attaches
    unsigned char* regOut;           // [P]: set for the points that registered in this round
    int* owner[3];                   // the decision's owner arrays (scratch): only the entries of this round's candidates are touched
    const int* curList;              // the frame's current points (cs_register_list_current_dev) and their count: who else wanted a feature
    const int* curCount;
    int curCap;
    int* counts;                     // [4] (accumulating): features attached, points registered, conflicts, sweeps that did not settle
    const int* listCount;            // null, or k_revisit_list's count: 0 = nobody is visited again (the usual round): leave at once
    int* nextList;                   // null, or the NEXT round's list [cap] (cleared to -1 before): a point that registered here and holds a
    int* nextCount;                  // feature in a later loop appends itself (what k_revisit_list would find), *nextCount counts them
    int* nextLoopW;                  // = nextLoop, written for the appended points
    int* overflow;                   // null, or where the points beyond the next list are counted
    int debug;                       // cs_debug_set("merge_print", 1): the launch prints where its time went
};
constexpr int RV_MAX_ROWS = 1024;
// what the walks of every round read, for the launch of one round (k_revisit_decide) and for the one that plays them all (k_revisit_rounds):
// the tables, the owner arrays out of the decision's scratch, where the points beyond the next list are counted.  A round's own list and the
// next one's (list, listCount, nextList, nextCount) are the caller's; the ranges (cameras, rows, kinds) it has checked.
inline int rv_fill(const char* who, RvArgs& A, int nCams, int N, int P, int cap, int mapBase, int kinds, int* d_nextLoop, int* d_visitLoop,
                   const int* d_slot, const int* d_flags, const unsigned char* d_mergeable, const unsigned char* d_mapFlags, int* d_pointFeat,
                   int* const* d_slot2map, unsigned char* d_attached, unsigned char* d_regOut, void* d_decideScratch, const int* d_curList,
                   const int* d_curCount, int curCap, int* d_counts, int* d_overflow) {
    if (!d_nextLoop || !d_visitLoop || !d_slot || !d_flags || !d_mergeable || !d_mapFlags || !d_pointFeat || !d_slot2map || !d_attached || !d_regOut ||
        !d_decideScratch || !d_curList || !d_curCount) {
        cs_set_error("%s: bad arguments (every table of the walks)", who);
        return CS_ERR_INVALID;
    }
    for (int c = 0; c < nCams; ++c) {
        if (!d_slot2map[c]) {
            cs_set_error("%s: null slot2map of camera %d", who, c);
            return CS_ERR_INVALID;
        }
        A.slot2map[c] = d_slot2map[c];
    }
    A.nCams = nCams, A.N = N, A.P = P, A.cap = cap, A.mapBase = mapBase, A.kinds = kinds, A.nextLoop = d_nextLoop, A.visitLoop = d_visitLoop;
    A.slot = d_slot, A.flags = d_flags, A.mergeable = d_mergeable, A.mapFlags = d_mapFlags, A.pointFeat = d_pointFeat;
    A.attached = d_attached, A.regOut = d_regOut, A.curList = d_curList, A.curCount = d_curCount, A.curCap = curCap, A.counts = d_counts;
    A.nextLoopW = d_nextLoop, A.overflow = d_overflow;
    A.debug = cs_debug_get(CS_DBG_MERGE_PRINT) == 1;
    int* scr = rd_scratch_owners(d_decideScratch, nCams, P);   // (cs_register_decide_kinds_dev's carve-up: head | code | base | owner x 3 | ...)
    for (int k = 0; k < 3; ++k) A.owner[k] = scr, scr += (size_t)nCams * N;
    return CS_OK;
}
// a round's list and the next round's: RvArgs' own fields, or (k_revisit_rounds) the round's slices of the frame's lists
struct RvRound {
    const int* list;
    const int* listCount;
    int* nextList;
    int* nextCount;
};
__device__ __forceinline__ RvRound rv_round_of(const RvArgs& A) { return RvRound{A.list, A.listCount, A.nextList, A.nextCount}; }
// owner array k mod 3 (selected, not indexed: a caller's own copy of the arguments then stays in registers)
__device__ __forceinline__ int* rv_owner(const RvArgs& A, int k) {
    const int r = k % 3;
    return r == 0 ? A.owner[0] : (r == 1 ? A.owner[1] : A.owner[2]);
}
// ---- a row's pieces: the same code whether a thread keeps its one row in registers (rv_decide_rows) or loops over several rows whose state
// waits in LDS between the barriers (rv_decide_rows_looped)
// the row's loads in three rounds (the point's flags, its loop and every camera's entry together; then who owns the candidates; then those
// owners' state) instead of up to four dependent loads per camera one camera after the other: the launch is a handful of rows' latency.
// Leaves the row's codes and base (-1: the row does not walk), clears its candidates' owners, counts the conflicts it can see already.
template <int MC>
__device__ __forceinline__ void rv_row_build(const RvArgs& A, int p, int (&code)[MC], int& base, int& nConf) {
    const int C = A.nCams;
    int kind = -1;
    base = -1;
#pragma unroll
    for (int i = 0; i < MC; ++i) code[i] = -1;
    int pfv[MC], slv[MC], flv[MC], own[MC];
    unsigned char mgv[MC];
    {
        const bool pv = p >= 0 && p < A.P;
        const size_t pr = pv ? (size_t)p : 0;
        const unsigned char fl = A.mapFlags[pr] & (CS_MAP_DYNAMIC | CS_MAP_FALSE | CS_MAP_UNCERTAIN);
        const int nl = A.nextLoop[pr];
#pragma unroll
        for (int i = 0; i < MC; ++i) {
            const size_t k = pr * C + (i < C ? i : 0);
            pfv[i] = A.pointFeat[k], slv[i] = A.slot[k], flv[i] = A.flags[k], mgv[i] = A.mergeable[k];
        }
        if (pv) {
            kind = (fl == 0 && (A.kinds & 1)) ? 0 : ((fl == CS_MAP_DYNAMIC && (A.kinds & 2)) ? 1 : -1);
            if (kind >= 0) base = (nl * A.P + p) * C;
        }
    }
    if (base >= 0) {
#pragma unroll
        for (int i = 0; i < MC; ++i) {
            const bool cand = i < C && pfv[i] < 0 && slv[i] >= 0 && slv[i] < A.N && ((flv[i] >> 1) & 1) == kind;   // :736-737; nothing found / the other type
            if (!cand) slv[i] = -1;
            // (the owner as a row of the pass; a point of the map below mapBase carries the feature all the same: A.P, "mapped, not one of ours")
            const int raw = cand ? A.slot2map[i][slv[i]] : -1;
            own[i] = raw < 0 ? -1 : (raw >= A.mapBase ? raw - A.mapBase : A.P);
        }
        int oAtt[MC], oPf[MC], oLoop[MC];
#pragma unroll
        for (int i = 0; i < MC; ++i) {
            const bool look = slv[i] >= 0 && own[i] >= 0 && own[i] < A.P;
            const size_t ko = (size_t)(look ? own[i] : 0) * C + (i < C ? i : 0);
            oAtt[i] = look ? A.attached[ko] : 0, oPf[i] = look ? A.pointFeat[ko] : -1, oLoop[i] = look ? A.visitLoop[look ? own[i] : 0] : 0;
        }
#pragma unroll
        for (int i = 0; i < MC; ++i) {
            if (slv[i] < 0) continue;
            const int sl = slv[i];
            int c = i * A.N + sl;
            if (own[i] >= 0) {
                c |= RD_INIT_MAPPED;
                // mapped NOW.  Was it mapped when this visit takes place?  Not if a later-ordered visit of this frame attached it.
                if (own[i] < A.P && oAtt[i] && oPf[i] == sl && (oLoop[i] * A.P + own[i]) * C + i > base + i) ++nConf;
            } else if (mgv[i] == 1) {
                c |= RD_CAN_MERGE;
            }
            code[i] = c;
        }
#pragma unroll
        for (int i = 0; i < MC; ++i)
            if (code[i] >= 0) rd_st(A.owner[0] + (code[i] & RD_FEAT), RD_INF), rd_st(A.owner[1] + (code[i] & RD_FEAT), RD_INF), rd_st(A.owner[2] + (code[i] & RD_FEAT), RD_INF);
    }
}
// the three steps of a Jacobi sweep (the decision's recursion: rd_resolve runs its sweeps on these too), a barrier between them
template <int MC>
__device__ __forceinline__ void rv_row_clear(const int (&code)[MC], int base, int* clear) {
    if (base < 0) return;
#pragma unroll
    for (int i = 0; i < MC; ++i)
        if (code[i] >= 0) rd_st(clear + (code[i] & RD_FEAT), RD_INF);
}
template <int MC>
__device__ __forceinline__ void rv_row_claim(const int (&code)[MC], int base, const int* prev, int* next) {
    if (base < 0) return;
    bool go = true;
#pragma unroll
    for (int i = 0; i < MC; ++i) {
        if (go && code[i] >= 0) {
            const int ord = base + i, f = code[i] & RD_FEAT;
            if ((code[i] & RD_INIT_MAPPED) || rd_ld(prev + f) < ord) go = false;
            else if (code[i] & RD_CAN_MERGE) atomicMin(&next[f], ord);
        }
    }
}
template <int MC>
__device__ __forceinline__ int rv_row_changed(const int (&code)[MC], int base, const int* prev, const int* next) {
    int ch = 0;
    if (base < 0) return ch;
#pragma unroll
    for (int i = 0; i < MC; ++i)
        if (code[i] >= 0) ch |= rd_ld(next + (code[i] & RD_FEAT)) != rd_ld(prev + (code[i] & RD_FEAT));
    return ch;
}
// what the round attached, for the conflict count's scan (the first 256)
struct RvAttached {
    int cam[256], sl[256], key[256], n;
};
// attach (the owners in `fin` are final); a row that registered marks itself and joins the next round's list
template <int MC>
__device__ __forceinline__ void rv_row_attach(const RvArgs& A, const RvRound& Rd, int p, const int (&code)[MC], int base, const int* fin, RvAttached& S, int& nAtt,
                                              int& nReg) {
    if (base < 0) return;
    const int C = A.nCams;
    bool go = true, reg = false;
#pragma unroll
    for (int i = 0; i < MC; ++i) {
        if (go && code[i] >= 0) {
            const int ord = base + i, f = code[i] & RD_FEAT, own = rd_ld(fin + f);
            if ((code[i] & RD_INIT_MAPPED) || own < ord) {
                go = false;
            } else if ((code[i] & RD_CAN_MERGE) && own == ord) {
                const int s2 = f - i * A.N;
                A.slot2map[i][s2] = A.mapBase + p;
                A.pointFeat[(size_t)p * C + i] = s2;
                A.attached[(size_t)p * C + i] = 1;
                reg = true, ++nAtt;
                const int q = atomicAdd(&S.n, 1);
                if (q < 256) S.cam[q] = i, S.sl[q] = s2, S.key[q] = ord;
            }
        }
    }
    if (reg) {
        ++nReg;
        const int last = A.nextLoop[p];
        A.regOut[p] = 1, A.visitLoop[p] = last;
        if (Rd.nextList) {
            int b = -1;
            for (int c = C - 1; c > last; --c)
                if (A.pointFeat[(size_t)p * C + c] >= 0) b = c;
            if (b >= 0) {
                const int q = atomicAdd(Rd.nextCount, 1);
                if (q < A.cap) Rd.nextList[q] = p, A.nextLoopW[p] = b;
                else if (A.overflow) atomicAdd(A.overflow, 1);
            }
        }
    }
}
// a feature attached here was unmapped until now: a LATER-ordered visit of this frame that had it as its candidate walked past it (it
// could not take it) and went on to other cameras -- in the reference's order that walk ends at it.  Counted where that walk attached
// something behind it (what it did there would not have happened).  q: a current point, qs: its candidates' slots.
template <int MC>
__device__ __forceinline__ void rv_conflicts_of(const RvArgs& A, int q, const int (&qs)[MC], const RvAttached& S, int nA, int& nConf) {
    const int C = A.nCams;
    // does ANY of the round's attachments name one of q's candidates?  (almost never: only then is q's row of features looked at)
    bool any = false;
    for (int a = 0; a < nA && !any; ++a) {
        const int i = S.cam[a], sl = S.sl[a];
#pragma unroll
        for (int t = 0; t < MC; ++t) any |= t == i && qs[t] == sl;
    }
    if (!any) return;
    int qp[MC];
    unsigned qatt = 0;
#pragma unroll
    for (int i = 0; i < MC; ++i) {
        const size_t kq = (size_t)q * C + (i < C ? i : 0);
        qp[i] = A.pointFeat[kq];
        if (i < C && A.attached[kq]) qatt |= 1u << i;
    }
    int lq = -1;   // the loop of q's (first) visit in this frame
#pragma unroll
    for (int i = MC - 1; i >= 0; --i)
        if (i < C && qp[i] >= 0 && !((qatt >> i) & 1u)) lq = i;
    if (lq < 0) return;
    for (int a = 0; a < nA; ++a) {
        const int i = S.cam[a], sl = S.sl[a];
        int qsi = -1, qpi = 0;
#pragma unroll
        for (int t = 0; t < MC; ++t)
            if (t == i) qsi = qs[t], qpi = qp[t];
        if (qsi != sl || qpi >= 0) continue;
        if ((lq * A.P + q) * C + i <= S.key[a]) continue;
        if ((qatt >> (i + 1)) != 0u) ++nConf;   // it attached something in a camera behind the one it walked past
    }
}
// MC: the cameras the row arrays are sized for (8 or RD_MAX_CAMS).  A thread per listed row.  Preconditions, the caller's: the workgroup
// has at least as many threads as the list has LISTED rows, and the entries of the list behind the listed ones, up to A.cap, are -1 (the
// kernels that build a list fill it so): thread j reads list[j] for every j < A.cap and takes a negative entry for "no row".  (The looped
// form below is handed the listed count and reads no entry behind it.)
template <int MC>
__device__ __forceinline__ void rv_decide_rows(const RvArgs& A, const RvRound& Rd) {
    __shared__ int sChanged;
    __shared__ RvAttached sAtt;
    const int j = threadIdx.x, C = A.nCams;
    const long long tD0 = A.debug ? wall_clock64() : 0;
    long long tD1 = 0, tD2 = 0, tD3 = 0;
    const int p = j < A.cap ? Rd.list[j] : -1;
    int code[MC], base = -1, nConf = 0;
    if (j == 0) sAtt.n = 0;
    // the conflict count's scan (at the end) compares every current point's candidates with what this round attached: the candidate rows do
    // not change in this launch, so a thread asks for its (up to two) current points' rows NOW -- the loads travel while the walks are built
    // and swept -- and the scan is register compares (it was 13 us of three dependent rounds of loads behind the attach, as much as the walks)
    const int nCurPre = *A.curCount < A.curCap ? *A.curCount : A.curCap;
    int preQ[2], preS[2][MC];
#pragma unroll
    for (int u = 0; u < 2; ++u) {
        const int e = j + u * (int)blockDim.x;
        preQ[u] = e < nCurPre ? A.curList[e] : -1;
        if (preQ[u] >= A.P) preQ[u] = -1;
#pragma unroll
        for (int i = 0; i < MC; ++i) preS[u][i] = preQ[u] >= 0 ? A.slot[(size_t)preQ[u] * C + (i < C ? i : 0)] : -1;
    }
    rv_row_build<MC>(A, p, code, base, nConf);
    __syncthreads();   // (ONE workgroup: its barrier orders the agent-scope accesses above -- an agent-scope fence here writes the XCD's L2 back, tracker's lines and all: 30-70 us a launch)
    if (A.debug) tD1 = wall_clock64();
    // Jacobi sweeps among the round's visits (the decision's recursion, one workgroup)
    int k = 0;
    const int* fin = A.owner[0];
    bool settled = false;
    for (; k < 32; ++k) {
        const int* prev = rv_owner(A, k);
        int* next = rv_owner(A, k + 1);
        int* clear = rv_owner(A, k + 2);
        if (j == 0) sChanged = 0;
        rv_row_clear<MC>(code, base, clear);
        __syncthreads();
        rv_row_claim<MC>(code, base, prev, next);
        __syncthreads();
        if (rv_row_changed<MC>(code, base, prev, next)) sChanged = 1;
        __syncthreads();
        fin = next;
        const int chg = sChanged;
        __syncthreads();
        if (!chg) {
            settled = true;
            break;
        }
    }
    if (A.debug) tD2 = wall_clock64();
    int nAtt = 0, nReg = 0;
    rv_row_attach<MC>(A, Rd, p, code, base, fin, sAtt, nAtt, nReg);
    __syncthreads();
    if (A.debug) tD3 = wall_clock64();
    const int nA = sAtt.n < 256 ? sAtt.n : 256;
    if (nA > 0) {
        const int nCur = nCurPre;
        for (int e = j, u = 0; e < nCur; e += (int)blockDim.x, ++u) {
            const int q = u == 0 ? preQ[0] : (u == 1 ? preQ[1] : A.curList[e]);
            if (q < 0 || q >= A.P) continue;
            int qs[MC];
#pragma unroll
            for (int i = 0; i < MC; ++i) qs[i] = u == 0 ? preS[0][i] : (u == 1 ? preS[1][i] : A.slot[(size_t)q * C + (i < C ? i : 0)]);
            rv_conflicts_of<MC>(A, q, qs, sAtt, nA, nConf);
        }
    }
    if (A.debug && j == 0)
        printf("k_revisit_decide: rows %d; build %lld us, %d sweeps %lld us, attach %lld us (%d attached), scan %lld us\n", Rd.listCount ? *Rd.listCount : -1,
               (tD1 - tD0) / 100, k + 1, (tD2 - tD1) / 100, (tD3 - tD2) / 100, nA, (wall_clock64() - tD3) / 100);
    if (A.counts) {
        if (nAtt) atomicAdd(A.counts, nAtt);
        if (nReg) atomicAdd(A.counts + 1, nReg);
        if (nConf) atomicAdd(A.counts + 2, nConf);
        if (j == 0 && !settled) atomicAdd(A.counts + 3, 1);
    }
}
// The same round for a list LONGER than the workgroup (NT threads, n rows, n > NT: the bootstrap frames).  A thread loops over rows
// tid, tid + NT, ... inside every phase, between the same barriers; a row's codes and base wait in LDS (rowCode [MC][RV_MAX_ROWS],
// rowBase [RV_MAX_ROWS]: camera-major, so a wave's rows are neighbouring words).  The sweeps reach the same fixed point however rows map to
// threads, the counters are sums, the next list is a set.  The current points' candidates are read when the scan needs them.
template <int MC, int NT>
__device__ __forceinline__ void rv_decide_rows_looped(const RvArgs& A, const RvRound& Rd, int n, int* rowCode, int* rowBase) {
    __shared__ int sChanged;
    __shared__ RvAttached sAtt;
    const int tid = threadIdx.x, C = A.nCams;
    int code[MC], base, nConf = 0;
    if (tid == 0) sAtt.n = 0;
    for (int j = tid; j < n; j += NT) {
        rv_row_build<MC>(A, Rd.list[j], code, base, nConf);
        rowBase[j] = base;
#pragma unroll
        for (int i = 0; i < MC; ++i) rowCode[i * RV_MAX_ROWS + j] = code[i];
    }
    __syncthreads();
    int k = 0;
    const int* fin = A.owner[0];
    bool settled = false;
    for (; k < 32; ++k) {
        const int* prev = rv_owner(A, k);
        int* next = rv_owner(A, k + 1);
        int* clear = rv_owner(A, k + 2);
        if (tid == 0) sChanged = 0;
        for (int j = tid; j < n; j += NT) {
#pragma unroll
            for (int i = 0; i < MC; ++i) code[i] = rowCode[i * RV_MAX_ROWS + j];
            rv_row_clear<MC>(code, rowBase[j], clear);
        }
        __syncthreads();
        for (int j = tid; j < n; j += NT) {
#pragma unroll
            for (int i = 0; i < MC; ++i) code[i] = rowCode[i * RV_MAX_ROWS + j];
            rv_row_claim<MC>(code, rowBase[j], prev, next);
        }
        __syncthreads();
        int ch = 0;
        for (int j = tid; j < n; j += NT) {
#pragma unroll
            for (int i = 0; i < MC; ++i) code[i] = rowCode[i * RV_MAX_ROWS + j];
            ch |= rv_row_changed<MC>(code, rowBase[j], prev, next);
        }
        if (ch) sChanged = 1;
        __syncthreads();
        fin = next;
        const int chg = sChanged;
        __syncthreads();
        if (!chg) {
            settled = true;
            break;
        }
    }
    int nAtt = 0, nReg = 0;
    for (int j = tid; j < n; j += NT) {
#pragma unroll
        for (int i = 0; i < MC; ++i) code[i] = rowCode[i * RV_MAX_ROWS + j];
        rv_row_attach<MC>(A, Rd, Rd.list[j], code, rowBase[j], fin, sAtt, nAtt, nReg);
    }
    __syncthreads();
    const int nA = sAtt.n < 256 ? sAtt.n : 256;
    if (nA > 0) {
        const int nCur = *A.curCount < A.curCap ? *A.curCount : A.curCap;
        for (int e = tid; e < nCur; e += NT) {
            const int q = A.curList[e];
            if (q < 0 || q >= A.P) continue;
            int qs[MC];
#pragma unroll
            for (int i = 0; i < MC; ++i) qs[i] = A.slot[(size_t)q * C + (i < C ? i : 0)];
            rv_conflicts_of<MC>(A, q, qs, sAtt, nA, nConf);
        }
    }
    if (A.debug && tid == 0) printf("k_revisit_rounds: rows %d in turns of %d; %d sweeps, %d attached\n", n, NT, k + 1, nA);
    if (A.counts) {
        if (nAtt) atomicAdd(A.counts, nAtt);
        if (nReg) atomicAdd(A.counts + 1, nReg);
        if (nConf) atomicAdd(A.counts + 2, nConf);
        if (tid == 0 && !settled) atomicAdd(A.counts + 3, 1);
    }
}

}  // namespace
