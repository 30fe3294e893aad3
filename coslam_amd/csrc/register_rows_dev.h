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
// MC: the cameras the row arrays are sized for (8 or MC: 16 cameras' worth of registers per thread spill at 1024 threads)
template <int MC>
__device__ __forceinline__ void rv_decide_rows(const RvArgs& A) {
    __shared__ int sChanged, sAttCam[256], sAttSl[256], sAttKey[256], sNAtt;
    const int j = threadIdx.x, C = A.nCams;
    const long long tD0 = A.debug ? wall_clock64() : 0;
    long long tD1 = 0, tD2 = 0, tD3 = 0;
    const int p = j < A.cap ? A.list[j] : -1;
    int code[MC], base = -1, kind = -1, nConf = 0;
#pragma unroll
    for (int i = 0; i < MC; ++i) code[i] = -1;
    if (j == 0) sNAtt = 0;
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
    // the row's loads in three rounds (the point's flags, its loop and every camera's entry together; then who owns the candidates; then those
    // owners' state) instead of up to four dependent loads per camera one camera after the other: the launch is a handful of rows' latency
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
            own[i] = cand ? A.slot2map[i][slv[i]] - A.mapBase : -1;
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
    __syncthreads();   // (ONE workgroup: its barrier orders the agent-scope accesses above -- an agent-scope fence here writes the XCD's L2 back, tracker's lines and all: 30-70 us a launch)
    if (A.debug) tD1 = wall_clock64();
    // Jacobi sweeps among the round's visits (k_decide_settle's recursion, one workgroup)
    int k = 0;
    const int* fin = A.owner[0];
    bool settled = false;
    for (; k < 32; ++k) {
        const int* prev = A.owner[k % 3];
        int* next = A.owner[(k + 1) % 3];
        int* clear = A.owner[(k + 2) % 3];
        if (j == 0) sChanged = 0;
        if (base >= 0) {
#pragma unroll
            for (int i = 0; i < MC; ++i)
                if (code[i] >= 0) rd_st(clear + (code[i] & RD_FEAT), RD_INF);
        }
        __syncthreads();
        if (base >= 0) {
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
        __syncthreads();
        if (base >= 0) {
            int ch = 0;
#pragma unroll
            for (int i = 0; i < MC; ++i)
                if (code[i] >= 0) ch |= rd_ld(next + (code[i] & RD_FEAT)) != rd_ld(prev + (code[i] & RD_FEAT));
            if (ch) sChanged = 1;
        }
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
    // attach (the owners in `fin` are final)
    bool reg = false;
    int nAtt = 0;
    if (base >= 0) {
        bool go = true;
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
                    const int q = atomicAdd(&sNAtt, 1);
                    if (q < 256) sAttCam[q] = i, sAttSl[q] = s2, sAttKey[q] = ord;
                }
            }
        }
        if (reg) {
            const int last = A.nextLoop[p];
            A.regOut[p] = 1, A.visitLoop[p] = last;
            if (A.nextList) {
                int b = -1;
                for (int c = C - 1; c > last; --c)
                    if (A.pointFeat[(size_t)p * C + c] >= 0) b = c;
                if (b >= 0) {
                    const int q = atomicAdd(A.nextCount, 1);
                    if (q < A.cap) A.nextList[q] = p, A.nextLoopW[p] = b;
                    else if (A.overflow) atomicAdd(A.overflow, 1);
                }
            }
        }
    }
    __syncthreads();
    // a feature attached here was unmapped until now: a LATER-ordered visit of this frame that had it as its candidate walked past it (it
    // could not take it) and went on to other cameras -- in the reference's order that walk ends at it.  Counted where that walk attached
    // something behind it (what it did there would not have happened).
    if (A.debug) tD3 = wall_clock64();
    const int nA = sNAtt < 256 ? sNAtt : 256;
    if (nA > 0) {
        const int nCur = nCurPre;
        for (int e = j, u = 0; e < nCur; e += (int)blockDim.x, ++u) {
            const int q = u < 2 ? preQ[u < 2 ? u : 0] : A.curList[e];
            if (q < 0 || q >= A.P) continue;
            int qs[MC];
#pragma unroll
            for (int i = 0; i < MC; ++i) qs[i] = u == 0 ? preS[0][i] : (u == 1 ? preS[1][i] : A.slot[(size_t)q * C + (i < C ? i : 0)]);
            // does ANY of the round's attachments name one of q's candidates?  (almost never: only then is q's row of features looked at)
            bool any = false;
            for (int a = 0; a < nA && !any; ++a) {
                const int i = sAttCam[a], sl = sAttSl[a];
#pragma unroll
                for (int t = 0; t < MC; ++t) any |= t == i && qs[t] == sl;
            }
            if (!any) continue;
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
            if (lq < 0) continue;
            for (int a = 0; a < nA; ++a) {
                const int i = sAttCam[a], sl = sAttSl[a];
                int qsi = -1, qpi = 0;
#pragma unroll
                for (int t = 0; t < MC; ++t)
                    if (t == i) qsi = qs[t], qpi = qp[t];
                if (qsi != sl || qpi >= 0) continue;
                if ((lq * A.P + q) * C + i <= sAttKey[a]) continue;
                if ((qatt >> (i + 1)) != 0u) ++nConf;   // it attached something in a camera behind the one it walked past
            }
        }
    }
    if (A.debug && j == 0)
        printf("k_revisit_decide: rows %d; build %lld us, %d sweeps %lld us, attach %lld us (%d attached), scan %lld us\n", A.listCount ? *A.listCount : -1,
               (tD1 - tD0) / 100, k + 1, (tD2 - tD1) / 100, (tD3 - tD2) / 100, nA, (wall_clock64() - tD3) / 100);
    if (A.counts) {
        if (nAtt) atomicAdd(A.counts, nAtt);
        if (reg) atomicAdd(A.counts + 1, 1);
        if (nConf) atomicAdd(A.counts + 2, nConf);
        if (j == 0 && !settled) atomicAdd(A.counts + 3, 1);
    }
}

}  // namespace
