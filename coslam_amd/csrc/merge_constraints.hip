// merge_constraints.hip -- the merge's bundle-adjustment problem and its MergeInfo list on the device (gfx950, wave64), DESIGN 3.22.
//
// Replaces MergeCameraGroup::genMergeInfoVer2 (src/app/SL_MergeCameraGroup.cpp:557-725) up to the solver call (:646) and behind it (:681-722),
// with its helpers getCamIdsInBothGroups (:489-511), getCorresFeatPtsAndMapPts (:762-811), checkMergeMapPoints (:425-467), mergeMapPoints
// (:468-488, emitted as a list, not applied), getUnMergedFeatureTracks (:812-882), getCorresFeatPtsInPrevSelfKeyPoses (:726-761) and
// getRigidTransFromToWithEMat (:1211-1219).  Everything it reads lives on the device: the current key frame's slot tables, the feature
// references with the history's linked segments, the history's pixels and poses, the map.  It writes only the handle's own buffers;
// k_merge_apply_map is the one kernel here that writes the live tables: the merge list and the solved points applied.
//
// It runs once per merge, so it is ONE workgroup of 1024 lanes that walks the reference's steps in order, a barrier between them; every
// output position comes from a scan (matches -> tracks -> views; tracks -> points -> measurements, in reverse track order) or from ballots
// (the stable counting sort of the unmerged candidates by numVisCam, 1..16: the rank inside a key is the count of earlier candidates with
// that key).  No atomic decides an order: the two that are used form a MAXIMUM of view indices ("the last track that holds the feature") and
// an OR of bits ("is an m1"), and a sum of integers; each gives the same value in whatever order the lanes arrive.  Doubles are only
// projected, compared and copied; the three largest errors are a selection, not a sum, until the final ((e0 + e1) + e2) / 3.
#include <vector>

#include "cs_common.h"
#include "dev_arena.h"
#include "history_view.h"

struct cs_merge_constraints {
    int device, nCams, N, maxMatches, maxMap, maxPoints, maxObs, maxViews;
    char* base;   // one allocation
    size_t bytes;
    cs_merge_constraints_buffers b;
    int4* trk;
    int *slotView, *candKey, *candRank, *candPt, *unm;
    unsigned* isM1;
    int* matches;   // [maxMatches][2]: cs_merge_constraints_assemble's copy of a host list
    CsStage stage;  // ... and the host side of that copy
    // cs_merge_constraints_apply_map_dev: winner tables (all -1 between calls) and the rows gathered from the pre-call table
    int *winSlot, *winRow, *winPt;   // [nCams][N], [maxMap][nCams], [maxMap]
    int4* gRef;                      // [maxViews]
    unsigned char* gStat;            // [maxViews]
    // the two solves (:646-647): the problem on the host, the existing robust BA's workspace, both results
    cs_ba* ba;
    int solved;   // 0: no solve since the last assembly, 1: both solves succeeded, -1: a solve failed
    int sC, sP, sObs;
    std::vector<double> hK, hXY, hR[2], hT[2], hM[2];
    std::vector<int> hPtr, hCam, hOut[2];
    cs_ba_stats stats[2];
};

namespace {

constexpr int MC_T = 1024, MC_WAVES = MC_T / 64, MC_MAX_CAMS = 16, MC_MAX_INFO = 48, MC_KEYS = 17;

struct McArgs {
    int nCams, N, H, head, stored, curFrame, segCap;
    int nMap, gId1, gId2, iCam, jCam, f1, f2, nMatch;
    double thres;
    const int4* featRef;     // [nMap][nCams] {slot, frame, first, seg}
    const int4* segPool;     // [nCams][segCap] {slot, last, first, next}
    const int* segCount;     // [nCams]
    const double *histXY, *histR, *histT;
    const double* mapPts;
    const cs_camera_groups* groups;
    const int2* matches;
    const double* xy[MC_MAX_CAMS];
    const int* state[MC_MAX_CAMS];
    const int* slot2map[MC_MAX_CAMS];
    const double* K[MC_MAX_CAMS];
    cs_merge_constraints_header* hdr;
    int4* trk;               // [maxMatches] {m1, m2, first view, views}
    cs_merge_view* views;
    int *slotView, *candKey, *candRank, *candPt, *unm;
    unsigned* isM1;
    double *Ks, *Rs, *Ts, *pts, *obsXY;
    int *pointMap, *obsPtr, *obsCam;
};

// exclusive scan of one int per lane over the workgroup; *total = the sum.  s_w: MC_WAVES + 1 ints of LDS.  Two barriers.
__device__ __forceinline__ int mc_block_scan(int v, int* s_w, int* total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int inc = v;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const int o = __shfl_up(inc, off, 64);
        if (lane >= off) inc += o;
    }
    __syncthreads();   // (s_w may still be read from the call before)
    if (lane == 63) s_w[wave] = inc;
    __syncthreads();
    int before = 0, all = 0;
#pragma unroll
    for (int w = 0; w < MC_WAVES; ++w) {
        const int t = s_w[w];
        before += w < wave ? t : 0;
        all += t;
    }
    *total = all;
    return before + inc - v;
}

// x into the descending triple (e0, e1, e2), as selects: a branchy insert becomes an indexed store into private memory
__device__ __forceinline__ void mc_top3(double x, double& e0, double& e1, double& e2) {
    const bool g0 = x > e0;
    const double d0 = g0 ? e0 : x;
    e0 = g0 ? x : e0;
    const bool g1 = d0 > e1;
    const double d1 = g1 ? e1 : d0;
    e1 = g1 ? d0 : e1;
    e2 = d1 > e2 ? d1 : e2;
}

__device__ __forceinline__ bool mc_cur_ref(const McArgs& A, int4 r) { return r.x >= 0 && r.x < A.N && r.y == A.f2; }

__device__ __forceinline__ int mc_ring_row(const McArgs& A, int f) { return (A.head - (A.curFrame - f) + A.H) % A.H; }

// the node of frame f1 on the chain behind a view of camera c (:741-748): its slot, or -1
__device__ __forceinline__ int mc_find_prev(const McArgs& A, int c, int slot, int first, int seg) {
    int hi = A.f2 - 1, lo = first, hops = 0;
    for (;;) {
        if (hi < A.f1) return -1;
        if (lo <= A.f1) return slot >= 0 && slot < A.N ? slot : -1;
        if (seg < 0 || seg >= A.segCap || hops >= A.segCap) return -1;   // the rule of merge_apply.hip's walk: a corrupt pool ends it
        const int4 g = A.segPool[(size_t)c * A.segCap + seg];
        ++hops;
        slot = g.x, hi = g.y, lo = g.z, seg = g.w;
    }
}

// one track: its views at f2, then the views at f1 behind them (:590), the duplicates of a (frame, camera) dropped (:631-634).
// WRITE: the measurements from obs on, and the marks of a merged track's views.  Returns views | measurements << 8 | f1 views << 16.
template <bool WRITE>
__device__ __forceinline__ int mc_track(const McArgs& A, int t, int nT, int nIds, const int* s_ids, const int* s_pos, int obs) {
    const bool merged = t < nT;
    const int4 tr = merged ? A.trk[t] : make_int4(A.unm[t - nT], -1, 0, nIds);
    unsigned seen2 = 0, seen1 = 0;
    int nv = 0, nMeas = 0, nPrev = 0;
    for (int pass = 0; pass < 2; ++pass)
        for (int k = 0; k < tr.w; ++k) {
            int c, slot, from;
            if (merged) {
                const cs_merge_view v = A.views[tr.z + k];
                c = v.cam, slot = v.slot, from = v.from;
            } else {
                c = s_ids[k], from = tr.x;
            }
            const int4 r = A.featRef[(size_t)from * A.nCams + c];
            if (!merged) {
                if (!mc_cur_ref(A, r)) continue;
                slot = r.x;
            }
            const unsigned bit = 1u << c;
            if (pass == 0) {
                ++nv;
                if (seen2 & bit) {
                    if (WRITE && merged) A.views[tr.z + k].flags |= CS_MERGE_VIEW_DETACHED;
                    continue;
                }
                seen2 |= bit;
                if (WRITE) {
                    A.obsCam[obs + nMeas] = s_pos[c];
                    A.obsXY[2 * (size_t)(obs + nMeas)] = A.xy[c][slot];
                    A.obsXY[2 * (size_t)(obs + nMeas) + 1] = A.xy[c][A.N + slot];
                }
                ++nMeas;
            } else {
                const int ps = mc_find_prev(A, c, slot, r.z, r.w);
                if (ps < 0) continue;
                ++nv, ++nPrev;
                if (WRITE && merged) A.views[tr.z + k].prevSlot = ps, A.views[tr.z + k].flags |= CS_MERGE_VIEW_PREV;
                if (seen1 & bit) {
                    if (WRITE && merged) A.views[tr.z + k].flags |= CS_MERGE_VIEW_PREV_DETACHED;
                    continue;
                }
                seen1 |= bit;
                if (WRITE) {
                    const double* row = A.histXY + ((size_t)c * A.H + mc_ring_row(A, A.f1)) * 2 * A.N;
                    A.obsCam[obs + nMeas] = nIds + s_pos[c];
                    A.obsXY[2 * (size_t)(obs + nMeas)] = row[ps];
                    A.obsXY[2 * (size_t)(obs + nMeas) + 1] = row[A.N + ps];
                }
                ++nMeas;
            }
        }
    return nv | nMeas << 8 | nPrev << 16;
}

__global__ __launch_bounds__(MC_T) void k_merge_assemble(McArgs A) {
    __shared__ int s_w[MC_WAVES + 1];
    __shared__ int s_ids[MC_MAX_CAMS], s_pos[MC_MAX_CAMS], s_n[4];
    __shared__ int s_cnt[MC_WAVES * MC_KEYS], s_run[MC_KEYS], s_base[MC_KEYS];
    __shared__ double s_top[MC_WAVES * 3];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, N = A.N;

    // ---- getCamIdsInBothGroups; the header starts as "nothing produced"
    if (tid == 0) {
        const cs_camera_groups& G = *A.groups;
        unsigned flags = 0;
        bool ok = G.groupNum >= 1 && G.groupNum <= 16 && A.gId1 >= 0 && A.gId1 < G.groupNum && A.gId2 >= 0 && A.gId2 < G.groupNum && A.gId1 != A.gId2;
        for (int q = 0; q < 2 && ok; ++q) {
            const int g = q ? A.gId2 : A.gId1, n = G.num[g];
            ok = n >= 1 && n <= 16;
            for (int i = 0; i < n && ok; ++i) {
                const int c = G.camIds[g][i];
                ok = c >= 0 && c < A.nCams;
                if (ok) flags |= 1u << c;
            }
        }
        int n = 0;
        for (int c = 0; c < MC_MAX_CAMS; ++c) {
            s_pos[c] = -1;
            if (ok && (flags >> c & 1)) s_pos[c] = n, s_ids[n++] = c;
        }
        s_n[0] = ok ? n : 0;
        s_n[1] = 0;   // f1 views
        int* hw = (int*)A.hdr;   // (written in place: a local copy indexed by c would live in private memory)
        for (int i = 0; i < (int)(sizeof(cs_merge_constraints_header) / sizeof(int)); ++i) hw[i] = 0;
        A.hdr->verdict = ok ? CS_MERGE_FEW : CS_MERGE_BAD_GROUPS;
        A.hdr->f1 = A.f1, A.hdr->f2 = A.f2, A.hdr->nCamIds = ok ? n : 0;
        for (int c = 0; c < 16; ++c) A.hdr->camIds[c] = ok && c < n ? s_ids[c] : -1;
    }
    for (int i = tid; i < A.nCams * N; i += MC_T) A.slotView[i] = -1;
    for (int i = tid; i < (A.nMap + 31) / 32; i += MC_T) A.isM1[i] = 0;
    __syncthreads();
    const int nIds = s_n[0];
    if (nIds == 0) return;

    // ---- 1. getCorresFeatPtsAndMapPts: matches -> tracks -> views, by scans; every track from the state as given
    int nT = 0, nV = 0;
    for (int b0 = 0; b0 < A.nMatch; b0 += MC_T) {
        const int i = b0 + tid;
        int m1 = -1, m2 = -1, nv = 0;
        if (i < A.nMatch) {
            const int2 mt = A.matches[i];
            if (mt.x >= 0 && mt.x < N && mt.y >= 0 && mt.y < N) {
                const int st1 = A.state[A.iCam][mt.x], st2 = A.state[A.jCam][mt.y];
                if ((st1 == 0 || st1 == 1) && (st2 == 0 || st2 == 1)) m1 = A.slot2map[A.iCam][mt.x], m2 = A.slot2map[A.jCam][mt.y];
            }
            if (m1 < 0 || m1 >= A.nMap || m2 < 0 || m2 >= A.nMap) m1 = m2 = -1;
        }
        if (m1 >= 0)
            for (int k = 0; k < nIds; ++k) {
                const int c = s_ids[k];
                nv += mc_cur_ref(A, A.featRef[(size_t)m1 * A.nCams + c]) ? 1 : 0;
                nv += mc_cur_ref(A, A.featRef[(size_t)m2 * A.nCams + c]) ? 1 : 0;
            }
        int totT, totV;
        const int t = nT + mc_block_scan(m1 >= 0 ? 1 : 0, s_w, &totT);
        int v = nV + mc_block_scan(nv, s_w, &totV);
        if (m1 >= 0) {
            A.trk[t] = make_int4(m1, m2, v, nv);
            for (int k = 0; k < nIds; ++k) {
                const int c = s_ids[k];
                for (int q = 0; q < 2; ++q) {
                    const int from = q ? m2 : m1;
                    const int4 r = A.featRef[(size_t)from * A.nCams + c];
                    if (!mc_cur_ref(A, r)) continue;
                    cs_merge_view e;
                    e.track = t, e.cam = c, e.slot = r.x, e.point = m1, e.from = from, e.flags = from != m1 ? CS_MERGE_VIEW_FROM_M2 : 0;
                    e.prevSlot = -1, e.reserved = 0;
                    A.views[v++] = e;
                }
            }
        }
        nT += totT, nV += totV;
    }
    __threadfence_block();
    __syncthreads();

    // ---- 2. checkMergeMapPoints: the three largest pixel distances of m1's projection from the views
    double e0 = -1, e1 = -1, e2 = -1;
    for (int v = tid; v < nV; v += MC_T) {
        const cs_merge_view e = A.views[v];
        const int c = e.cam, rs = mc_ring_row(A, A.f2);
        const double* R = A.histR + ((size_t)c * A.H + rs) * 9;
        const double* t = A.histT + ((size_t)c * A.H + rs) * 3;
        const double* K = A.K[c];
        const double* M = A.mapPts + 3 * (size_t)e.point;
        const double X = R[0] * M[0] + R[1] * M[1] + R[2] * M[2] + t[0];   // project (oracle/ref_shim/shim_impl.cpp)
        const double Y = R[3] * M[0] + R[4] * M[1] + R[5] * M[2] + t[1];
        const double Z = R[6] * M[0] + R[7] * M[1] + R[8] * M[2] + t[2];
        const double u = K[0] * X + K[1] * Y + K[2] * Z, w = K[3] * X + K[4] * Y + K[5] * Z, z = K[6] * X + K[7] * Y + K[8] * Z;
        const double dx = u / z - A.xy[c][e.slot], dy = w / z - A.xy[c][N + e.slot];
        mc_top3(sqrt(dx * dx + dy * dy), e0, e1, e2);   // dist2
    }
#pragma unroll 1
    for (int off = 1; off < 64; off <<= 1) {
        const double o0 = __shfl_xor(e0, off, 64), o1 = __shfl_xor(e1, off, 64), o2 = __shfl_xor(e2, off, 64);
        mc_top3(o0, e0, e1, e2), mc_top3(o1, e0, e1, e2), mc_top3(o2, e0, e1, e2);
    }
    if (lane == 0) s_top[3 * wave] = e0, s_top[3 * wave + 1] = e1, s_top[3 * wave + 2] = e2;
    __syncthreads();
    if (tid == 0) {
        double a0 = -1, a1 = -1, a2 = -1;
#pragma unroll 1
        for (int i = 0; i < 3 * MC_WAVES; ++i) mc_top3(s_top[i], a0, a1, a2);
        int verdict = CS_MERGE_FEW;
        double avg = 0;
        if (nT > 0 && nV >= 3) {
            avg = ((a0 + a1) + a2) / 3;
            verdict = avg > A.thres ? CS_MERGE_REJECT : CS_MERGE_OK;
        }
        A.hdr->verdict = verdict, A.hdr->avgErr = avg, A.hdr->nMergedTracks = nT, A.hdr->skippedMatches = A.nMatch - nT;
        s_n[2] = verdict;
    }
    __syncthreads();
    if (s_n[2] != CS_MERGE_OK) return;

    // ---- 3. mergeMapPoints, as the state the later steps see: a feature's point is the m1 of the LAST track that holds it
    for (int v = tid; v < nV; v += MC_T) atomicMax(&A.slotView[A.views[v].cam * N + A.views[v].slot], v);
    for (int t = tid; t < nT; t += MC_T) atomicOr(&A.isM1[A.trk[t].x >> 5], 1u << (A.trk[t].x & 31));
    if (tid < MC_KEYS) s_run[tid] = 0;
    __threadfence_block();
    __syncthreads();

    // ---- 4. getUnMergedFeatureTracks: candidates in camera and slot order, a stable counting sort by numVisCam descending
    const int nPos = nIds * N;
    for (int b0 = 0; b0 < nPos; b0 += MC_T) {
        const int p = b0 + tid;
        int key = 0, q = -1;
        if (p < nPos) {
            const int c = s_ids[p / N], s = p - (p / N) * N, st = A.state[c][s];
            if (st == 0 || st == 1) {
                const int sv = __hip_atomic_load(&A.slotView[c * N + s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // (written by atomics)
                q = sv >= 0 ? A.views[sv].point : A.slot2map[c][s];
                if (q < 0 || q >= A.nMap || (__hip_atomic_load(&A.isM1[q >> 5], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >> (q & 31) & 1)) q = -1;
            }
            if (q >= 0) {
                int vis = 0, inGroups = 0;
                for (int cc = 0; cc < A.nCams; ++cc) {
                    const bool cur = mc_cur_ref(A, A.featRef[(size_t)q * A.nCams + cc]);
                    vis += cur ? 1 : 0, inGroups += cur && s_pos[cc] >= 0 ? 1 : 0;
                }
                key = inGroups >= 1 ? vis : 0;   // a track without a view is never appended (:874)
            }
        }
        int mine = 0, cnt = 0;
        for (int k = 1; k < MC_KEYS; ++k) {
            const unsigned long long mask = __ballot(key == k);
            if (key == k) mine = __popcll(mask & ((1ull << lane) - 1));
            if (lane == k) cnt = __popcll(mask);
        }
        if (lane >= 1 && lane < MC_KEYS) s_cnt[wave * MC_KEYS + lane] = cnt;
        __syncthreads();
        if (p < nPos) {
            int r = -1;
            if (key > 0) {
                r = s_run[key] + mine;
                for (int w = 0; w < wave; ++w) r += s_cnt[w * MC_KEYS + key];
            }
            A.candKey[p] = key, A.candRank[p] = r, A.candPt[p] = q;
        }
        __syncthreads();
        if (tid >= 1 && tid < MC_KEYS) {
            int add = 0;
            for (int w = 0; w < MC_WAVES; ++w) add += s_cnt[w * MC_KEYS + tid];
            s_run[tid] += add;
        }
        __syncthreads();
    }
    if (tid == 0) {
        int sum = 0;
        for (int k = MC_KEYS - 1; k >= 1; --k) s_base[k] = sum, sum += s_run[k];
        const int cap = 20 * nT;
        s_n[3] = sum < cap ? sum : cap;
    }
    __syncthreads();
    const int nU = s_n[3];
    for (int p = tid; p < nPos; p += MC_T) {
        const int key = A.candKey[p];
        if (key <= 0) continue;
        const int r = s_base[key] + A.candRank[p];
        if (r < nU) A.unm[r] = A.candPt[p];
    }
    __threadfence_block();
    __syncthreads();

    // ---- 5. + 6. the views at f1, and the problem: tracks of more than one view in REVERSE order, by scans
    const int nTr = nT + nU;
    int P = 0, nObs = 0, nPrevMine = 0;
    for (int b0 = 0; b0 < nTr; b0 += MC_T) {
        const int j = b0 + tid, t = nTr - 1 - j;
        int keep = 0, nMeas = 0;
        if (j < nTr) {
            const int r = mc_track<false>(A, t, nT, nIds, s_ids, s_pos, 0);
            keep = (r & 255) > 1 ? 1 : 0, nMeas = keep ? (r >> 8 & 255) : 0, nPrevMine += r >> 16;
        }
        int totP, totO;
        const int pt = P + mc_block_scan(keep, s_w, &totP);
        const int ob = nObs + mc_block_scan(nMeas, s_w, &totO);
        if (keep) {
            const int m = t < nT ? A.trk[t].x : A.unm[t - nT];
            mc_track<true>(A, t, nT, nIds, s_ids, s_pos, ob);
            A.pointMap[pt] = m, A.obsPtr[pt] = ob;
            for (int q = 0; q < 3; ++q) A.pts[3 * (size_t)pt + q] = A.mapPts[3 * (size_t)m + q];
        }
        P += totP, nObs += totO;
    }
    if (nPrevMine) atomicAdd(&s_n[1], nPrevMine);
    // ---- the poses in the order of buildIdMapForSelfKeyPoses (:605-616)
    if (tid < 2 * nIds) {
        const int c = s_ids[tid % nIds], rs = mc_ring_row(A, tid < nIds ? A.f2 : A.f1);
        for (int q = 0; q < 9; ++q) A.Ks[9 * tid + q] = A.K[c][q], A.Rs[9 * tid + q] = A.histR[((size_t)c * A.H + rs) * 9 + q];
        for (int q = 0; q < 3; ++q) A.Ts[3 * tid + q] = A.histT[((size_t)c * A.H + rs) * 3 + q];
    }
    __syncthreads();
    if (tid == 0) {
        A.obsPtr[P] = nObs;
        A.hdr->nPose = 2 * nIds, A.hdr->P = P, A.hdr->nObs = nObs, A.hdr->nUnmerged = nU, A.hdr->nPrevViews = s_n[1], A.hdr->nMergeViews = nV;
    }
}

struct MiArgs {
    const cs_merge_constraints_header* hdrIn;
    cs_merge_constraints_header* hdr;
    const cs_camera_groups* groups;
    int gId1, gId2;
    const double *Rs, *Ts;
    cs_merge_info* info;
    unsigned char* valid;
    double *infoR, *infoT;
};

// :681-722, one lane per MergeInfo; getRigidTransFromTo as oracle/ref_shim/ref_glue_impl.cpp writes it: R = R2 R1^T, t = t2 - R t1
__global__ __launch_bounds__(64) void k_merge_info(MiArgs A) {
    const cs_merge_constraints_header& H = *A.hdrIn;
    const int i = threadIdx.x;
    const cs_camera_groups& G = *A.groups;
    bool ok = H.verdict == CS_MERGE_OK && H.nCamIds >= 1 && H.nCamIds <= 16 && H.nPose == 2 * H.nCamIds && G.groupNum >= 1 && G.groupNum <= 16 &&
              A.gId1 >= 0 && A.gId1 < G.groupNum && A.gId2 >= 0 && A.gId2 < G.groupNum;
    const int n1 = ok ? G.num[A.gId1] : 0, n2 = ok ? G.num[A.gId2] : 0;
    ok = ok && n1 >= 1 && n1 <= 16 && n2 >= 1 && n2 <= 16;
    const int nInfo = ok ? n2 + n1 - 1 + H.nCamIds : 0;
    if (i == 0) A.hdr->nInfo = nInfo;
    if (i >= nInfo) return;
    cs_merge_info e;
    if (i < n2) e = {H.f2, G.camIds[A.gId1][0], A.gId1, H.f2, G.camIds[A.gId2][i], A.gId2};
    else if (i < n2 + n1 - 1) e = {H.f2, G.camIds[A.gId1][i - n2 + 1], A.gId1, H.f2, G.camIds[A.gId2][0], A.gId2};
    else e = {H.f2, H.camIds[i - n2 - n1 + 1], -1, H.f1, H.camIds[i - n2 - n1 + 1], -1};
    int p = -1, q = -1;
    for (int k = 0; k < H.nCamIds; ++k) {
        if (H.camIds[k] == e.cam1) p = k;
        if (H.camIds[k] == e.cam2) q = k + (e.frame2 == H.f2 ? 0 : H.nCamIds);
    }
    A.info[i] = e;
    const bool valid = p >= 0 && q >= 0;   // (a camera of the record that is not in the order: cannot happen behind the assembly)
    A.valid[i] = valid ? 1 : 0;
    if (!valid) return;
    const double *R1 = A.Rs + 9 * p, *t1 = A.Ts + 3 * p, *R2 = A.Rs + 9 * q, *t2 = A.Ts + 3 * q;
    double R[9];
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) R[3 * r + c] = R2[3 * r] * R1[3 * c] + R2[3 * r + 1] * R1[3 * c + 1] + R2[3 * r + 2] * R1[3 * c + 2];
    for (int k = 0; k < 9; ++k) A.infoR[9 * i + k] = R[k];
    for (int r = 0; r < 3; ++r) A.infoT[3 * i + r] = t2[r] - (R[3 * r] * t1[0] + R[3 * r + 1] * t1[1] + R[3 * r + 2] * t1[2]);
}

struct MmArgs {
    int nCams, N, nMap, maxViews, maxPoints, applyPts;
    const cs_merge_constraints_header* hdr;
    const cs_merge_view* views;
    const int* pointMap;
    const double* solvedPts;
    int* slot2map[MC_MAX_CAMS];
    int* pointFeat;             // [nMap][nCams] or NULL
    int4* featRef;              // [nMap][nCams] {slot, frame, first, seg}
    unsigned char* refStatic;   // [nMap][nCams] or NULL
    double* mapPts;             // [nMap][3] (read only when applyPts)
    int* counts;                // [6] or NULL
    int *winSlot, *winRow, *winPt;
    int4* gRef;
    unsigned char* gStat;
};

__device__ __forceinline__ bool mm_view_ok(const MmArgs& A, const cs_merge_view& e) {
    return e.cam >= 0 && e.cam < A.nCams && e.slot >= 0 && e.slot < A.N && e.point >= 0 && e.point < A.nMap && e.from >= 0 && e.from < A.nMap;
}

__device__ __forceinline__ int mm_load(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }   // (written by atomics)

// mergeMapPoints (:468-488), the duplicate marks of :631-634 and the solved coordinates (:665-669) on the live tables, DESIGN 3.23.  One
// workgroup, four passes with a barrier between them: (1) every source row is gathered from the table as it stands and every entry bids for
// its slot (c, s), its row (m1, c) and its map row with its INDEX (atomicMax: "the last one wins" as an integer maximum); (2) the winners
// write; (3) the detached features, whichever entry came last; (4) the winner tables go back to -1 at the entries the lists named.
__global__ __launch_bounds__(MC_T) void k_merge_apply_map(MmArgs A) {
    __shared__ int s_n[3], s_cnt[6];
    const int tid = threadIdx.x, nC = A.nCams, N = A.N;
    if (tid == 0) {
        const int nV = A.hdr->nMergeViews, P = A.hdr->P;
        s_n[0] = A.hdr->verdict == CS_MERGE_OK ? 1 : 0;
        s_n[1] = nV < 0 ? 0 : nV > A.maxViews ? A.maxViews : nV;
        s_n[2] = !A.applyPts || P < 0 ? 0 : P > A.maxPoints ? A.maxPoints : P;
    }
    if (tid < 6) s_cnt[tid] = 0;
    __syncthreads();
    if (!s_n[0]) return;   // a verdict other than CS_MERGE_OK: nothing written, nothing counted
    const int nV = s_n[1], P = s_n[2];
    int applied = 0, moved = 0, detached = 0, prevMarked = 0, written = 0, lost = 0;

    // ---- 1. gather and bid
    for (int v = tid; v < nV; v += MC_T) {
        const cs_merge_view e = A.views[v];
        if (!mm_view_ok(A, e)) {
            ++lost;
            continue;
        }
        ++applied;
        const size_t src = (size_t)e.from * nC + e.cam;
        A.gRef[v] = A.featRef[src];
        A.gStat[v] = A.refStatic ? A.refStatic[src] : 0;
        atomicMax(&A.winSlot[e.cam * N + e.slot], v);
        atomicMax(&A.winRow[(size_t)e.point * nC + e.cam], v);
    }
    for (int i = tid; i < P; i += MC_T) {
        const int m = A.pointMap[i];
        if (m < 0 || m >= A.nMap) {
            ++lost;
            continue;
        }
        atomicMax(&A.winPt[m], i);
    }
    __threadfence_block();
    __syncthreads();

    // ---- 2. the winners write: slot2map[c][s] = m1; m1's reference in c = the gathered row of `from`
    for (int v = tid; v < nV; v += MC_T) {
        const cs_merge_view e = A.views[v];
        if (!mm_view_ok(A, e)) continue;
        const bool winS = mm_load(&A.winSlot[e.cam * N + e.slot]) == v, winR = mm_load(&A.winRow[(size_t)e.point * nC + e.cam]) == v;
        if (winS) A.slot2map[e.cam][e.slot] = e.point;
        if (winR) {
            const size_t dst = (size_t)e.point * nC + e.cam;
            A.featRef[dst] = A.gRef[v];
            if (A.refStatic) A.refStatic[dst] = A.gStat[v];
            if (A.pointFeat) A.pointFeat[dst] = e.slot;
            moved += e.from != e.point ? 1 : 0;
        }
        lost += winS && winR ? 0 : 1;
    }
    for (int i = tid; i < P; i += MC_T) {
        const int m = A.pointMap[i];
        if (m < 0 || m >= A.nMap) continue;
        if (mm_load(&A.winPt[m]) == i) {
            for (int q = 0; q < 3; ++q) A.mapPts[3 * (size_t)m + q] = A.solvedPts[3 * (size_t)i + q];
            ++written;
        } else
            ++lost;
    }
    __threadfence_block();
    __syncthreads();

    // ---- 3. `fp->mpt = 0`: a detached feature loses its point whatever entry named its slot last; the first to take the slot's winner
    // entry counts the feature (one per slot, whoever it is)
    for (int v = tid; v < nV; v += MC_T) {
        const cs_merge_view e = A.views[v];
        if (!mm_view_ok(A, e)) continue;
        if (e.flags & CS_MERGE_VIEW_DETACHED) {
            detached += atomicExch(&A.winSlot[e.cam * N + e.slot], -2) >= 0 ? 1 : 0;
            A.slot2map[e.cam][e.slot] = -1;
        }
        prevMarked += e.flags & CS_MERGE_VIEW_PREV_DETACHED ? 1 : 0;   // a node of a past frame has no owner entry here: counted only
    }
    __threadfence_block();
    __syncthreads();

    // ---- 4. the winner tables as they were
    for (int v = tid; v < nV; v += MC_T) {
        const cs_merge_view e = A.views[v];
        if (!mm_view_ok(A, e)) continue;
        A.winSlot[e.cam * N + e.slot] = -1;
        A.winRow[(size_t)e.point * nC + e.cam] = -1;
    }
    for (int i = tid; i < P; i += MC_T) {
        const int m = A.pointMap[i];
        if (m >= 0 && m < A.nMap) A.winPt[m] = -1;
    }
    if (applied) atomicAdd(&s_cnt[0], applied);
    if (moved) atomicAdd(&s_cnt[1], moved);
    if (detached) atomicAdd(&s_cnt[2], detached);
    if (prevMarked) atomicAdd(&s_cnt[3], prevMarked);
    if (written) atomicAdd(&s_cnt[4], written);
    if (lost) atomicAdd(&s_cnt[5], lost);
    __syncthreads();
    if (tid < 6 && A.counts) A.counts[tid] += s_cnt[tid];
}

}  // namespace

// the device block: the exported problem and lists, the assembly's work tables, the solve's results, the map update's tables
static void mc_layout(cs_merge_constraints* mc, CsArena& ar) {
    const size_t nM = mc->maxMatches, nP = mc->maxPoints, nO = mc->maxObs, nV = mc->maxViews, nS = (size_t)MC_MAX_CAMS * mc->N;
    cs_merge_constraints_buffers& B = mc->b;
    ar.take(B.header, 1), ar.take(B.views, nV), ar.take(B.Ks, 32 * 9), ar.take(B.Rs, 32 * 9), ar.take(B.Ts, 32 * 3), ar.take(B.pts, nP * 3);
    ar.take(B.pointMap, nP), ar.take(B.obsPtr, nP + 1), ar.take(B.obsCam, nO), ar.take(B.obsXY, nO * 2);
    ar.take(B.info, MC_MAX_INFO), ar.take(B.infoValid, MC_MAX_INFO), ar.take(B.infoR, MC_MAX_INFO * 9), ar.take(B.infoT, MC_MAX_INFO * 3);
    ar.take(mc->trk, nM), ar.take(mc->slotView, nS), ar.take(mc->candKey, nS), ar.take(mc->candRank, nS), ar.take(mc->candPt, nS);
    ar.take(mc->unm, 20 * nM), ar.take(mc->isM1, ((size_t)mc->maxMap + 31) / 32);
    ar.take(B.solvedRs, 32 * 9), ar.take(B.solvedTs, 32 * 3), ar.take(B.solvedPts, nP * 3), ar.take(B.outlier, nO);
    ar.take(mc->matches, nM * 2);
    ar.take(mc->winSlot, (size_t)mc->nCams * mc->N), ar.take(mc->winRow, (size_t)mc->maxMap * mc->nCams), ar.take(mc->winPt, mc->maxMap);
    ar.take(mc->gRef, nV), ar.take(mc->gStat, nV);
}

extern "C" cs_merge_constraints* cs_merge_constraints_create(int device, int nCams, int N, int maxMatches, int maxMap) {
    if (nCams < 1 || nCams > MC_MAX_CAMS || N < 1 || maxMatches < 1 || maxMap < 1 || maxMatches > (1 << 20) / 21) {
        cs_set_error("cs_merge_constraints_create: bad argument (nCams %d, N %d, maxMatches %d, maxMap %d)", nCams, N, maxMatches, maxMap);
        return nullptr;
    }
    cs_merge_constraints* mc = new cs_merge_constraints();
    mc->device = device, mc->nCams = nCams, mc->N = N, mc->maxMatches = maxMatches, mc->maxMap = maxMap;
    mc->maxPoints = 21 * maxMatches, mc->maxObs = 32 * mc->maxPoints, mc->maxViews = 32 * maxMatches;
    if (!cs_arena_alloc(device, mc->base, mc->bytes, [mc](CsArena& ar) { mc_layout(mc, ar); })) {
        cs_set_error("cs_merge_constraints_create: %zu bytes of device memory: %s", mc->bytes, hipGetErrorString(hipGetLastError()));
        delete mc;
        return nullptr;
    }
    cs_merge_constraints_buffers& B = mc->b;
    B.maxPoints = mc->maxPoints, B.maxObs = mc->maxObs, B.maxViews = mc->maxViews, B.maxInfo = MC_MAX_INFO;
    // the three winner tables: -1 once, every call restores what it named
    if (hipMemset(mc->winSlot, 0xFF, 4 * (size_t)nCams * N) != hipSuccess || hipMemset(mc->winRow, 0xFF, 4 * (size_t)maxMap * nCams) != hipSuccess ||
        hipMemset(mc->winPt, 0xFF, 4 * (size_t)maxMap) != hipSuccess) {
        cs_set_error("cs_merge_constraints_create: %s", hipGetErrorString(hipGetLastError()));
        (void)hipFree(mc->base);
        delete mc;
        return nullptr;
    }
    mc->ba = nullptr, mc->solved = 0, mc->sC = mc->sP = mc->sObs = 0;
    return mc;
}

extern "C" void cs_merge_constraints_destroy(cs_merge_constraints* mc) {
    if (!mc) return;
    if (mc->ba) cs_ba_destroy(mc->ba);
    if (mc->base) {
        (void)hipSetDevice(mc->device);
        mc->stage.drain();   // (the upload of the last assembly may still read its staging copy)
        (void)hipFree(mc->base);
    }
    delete mc;
}

extern "C" int cs_merge_constraints_assemble_dev(cs_merge_constraints* mc, const cs_track_history* h, void* hip_stream, const cs_merge_cam* cams,
                                                 const cs_feat_ref* d_featRef, int nMap, const double* d_mapPts, const cs_camera_groups* d_groups,
                                                 int gId1, int gId2, int maxiCam, int maxjCam, int f1, int f2, const int* d_matches, int nMatches) {
    const char* who = "cs_merge_constraints_assemble_dev";
    if (!mc || !h || !cams || !d_featRef || !d_mapPts || !d_groups || nMap < 0 || nMatches < 0 || (nMatches > 0 && !d_matches)) {
        cs_set_error("%s: bad arguments", who);
        return CS_ERR_INVALID;
    }
    CsHistView v;
    cs_history_view(h, &v);
    if (v.nCams != mc->nCams || v.N != mc->N) {
        cs_set_error("%s: the history has %d cameras x %d slots, the handle %d x %d", who, v.nCams, v.N, mc->nCams, mc->N);
        return CS_ERR_INVALID;
    }
    if (nMatches > mc->maxMatches || nMap > mc->maxMap) {
        cs_set_error("%s: %d matches / %d map rows, the handle was created for %d / %d", who, nMatches, nMap, mc->maxMatches, mc->maxMap);
        return CS_ERR_INVALID;
    }
    if (maxiCam < 0 || maxiCam >= v.nCams || maxjCam < 0 || maxjCam >= v.nCams || gId1 < 0 || gId1 >= 16 || gId2 < 0 || gId2 >= 16 || gId1 == gId2) {
        cs_set_error("%s: cameras %d / %d of %d, groups %d / %d", who, maxiCam, maxjCam, v.nCams, gId1, gId2);
        return CS_ERR_INVALID;
    }
    if (v.stored < 1 || f2 != v.lastFrame) {
        cs_set_error("%s: f2 = %d is not the history's newest frame (%d)", who, f2, v.stored < 1 ? -1 : v.lastFrame);
        return CS_ERR_INVALID;
    }
    if (f1 >= f2 || f2 - f1 >= v.stored) {
        cs_set_error("%s: the first-constrained frame %d is not behind frame %d inside the store (frames %d .. %d)", who, f1, f2,
                     v.lastFrame - v.stored + 1, v.lastFrame);
        return CS_ERR_INVALID;
    }
    McArgs A;
    memset(&A, 0, sizeof(A));
    A.nCams = v.nCams, A.N = v.N, A.H = v.H, A.head = v.head, A.stored = v.stored, A.curFrame = v.lastFrame, A.segCap = v.segCap;
    A.nMap = nMap, A.gId1 = gId1, A.gId2 = gId2, A.iCam = maxiCam, A.jCam = maxjCam, A.f1 = f1, A.f2 = f2, A.nMatch = nMatches, A.thres = 500.0;
    A.featRef = (const int4*)d_featRef, A.segPool = v.segPool, A.segCount = v.segCount, A.histXY = v.xy, A.histR = v.R, A.histT = v.t;
    A.mapPts = d_mapPts, A.groups = d_groups, A.matches = (const int2*)d_matches;
    for (int c = 0; c < v.nCams; ++c) {
        if (!cams[c].xy || !cams[c].state || !cams[c].slot2map || !cams[c].K) {
            cs_set_error("%s: null xy / state / slot2map / K in camera %d", who, c);
            return CS_ERR_INVALID;
        }
        A.xy[c] = cams[c].xy, A.state[c] = cams[c].state, A.slot2map[c] = cams[c].slot2map, A.K[c] = cams[c].K;
    }
    const cs_merge_constraints_buffers& B = mc->b;
    A.hdr = (cs_merge_constraints_header*)B.header, A.trk = mc->trk, A.views = (cs_merge_view*)B.views;
    A.slotView = mc->slotView, A.candKey = mc->candKey, A.candRank = mc->candRank, A.candPt = mc->candPt, A.unm = mc->unm, A.isM1 = mc->isM1;
    A.Ks = (double*)B.Ks, A.Rs = (double*)B.Rs, A.Ts = (double*)B.Ts, A.pts = (double*)B.pts, A.obsXY = (double*)B.obsXY;
    A.pointMap = (int*)B.pointMap, A.obsPtr = (int*)B.obsPtr, A.obsCam = (int*)B.obsCam;
    mc->solved = 0;
    CS_HIP(hipSetDevice(mc->device));
    hipLaunchKernelGGL(k_merge_assemble, dim3(1), dim3(MC_T), 0, (hipStream_t)hip_stream, A);
    CS_CHECK_LAUNCH();
    return CS_OK;
}

extern "C" int cs_merge_constraints_assemble(cs_merge_constraints* mc, const cs_track_history* h, void* hip_stream, const cs_merge_cam* cams,
                                             const cs_feat_ref* d_featRef, int nMap, const double* d_mapPts, const cs_camera_groups* d_groups, int gId1,
                                             int gId2, int maxiCam, int maxjCam, int f1, int f2, const int* h_matches, int nMatches) {
    if (!mc || nMatches < 0 || nMatches > mc->maxMatches || (nMatches > 0 && !h_matches)) {
        cs_set_error("cs_merge_constraints_assemble: %d matches, the handle was created for %d", nMatches, mc ? mc->maxMatches : 0);
        return CS_ERR_INVALID;
    }
    if (nMatches > 0) {
        CS_HIP(hipSetDevice(mc->device));
        int rc = mc->stage.begin((hipStream_t)hip_stream);
        if (rc == CS_OK) rc = mc->stage.upload((hipStream_t)hip_stream, mc->matches, h_matches, 8 * (size_t)nMatches);
        if (rc != CS_OK) return rc;
    }
    return cs_merge_constraints_assemble_dev(mc, h, hip_stream, cams, d_featRef, nMap, d_mapPts, d_groups, gId1, gId2, maxiCam, maxjCam, f1, f2,
                                             mc->matches, nMatches);
}

extern "C" int cs_merge_info_dev(cs_merge_constraints* mc, void* hip_stream, const cs_camera_groups* d_groups, int gId1, int gId2,
                                 const double* d_Rs, const double* d_Ts) {
    if (!mc || !d_groups || !d_Rs || !d_Ts) {
        cs_set_error("cs_merge_info_dev: bad arguments");
        return CS_ERR_INVALID;
    }
    MiArgs A;
    A.hdrIn = mc->b.header, A.hdr = (cs_merge_constraints_header*)mc->b.header, A.groups = d_groups, A.gId1 = gId1, A.gId2 = gId2;
    A.Rs = d_Rs, A.Ts = d_Ts, A.info = (cs_merge_info*)mc->b.info, A.valid = (unsigned char*)mc->b.infoValid;
    A.infoR = (double*)mc->b.infoR, A.infoT = (double*)mc->b.infoT;
    CS_HIP(hipSetDevice(mc->device));
    hipLaunchKernelGGL(k_merge_info, dim3(1), dim3(64), 0, (hipStream_t)hip_stream, A);
    CS_CHECK_LAUNCH();
    return CS_OK;
}

extern "C" int cs_merge_constraints_buffers_get(const cs_merge_constraints* mc, cs_merge_constraints_buffers* out) {
    if (!mc || !out) {
        cs_set_error("cs_merge_constraints_buffers_get: bad arguments");
        return CS_ERR_INVALID;
    }
    *out = mc->b;
    return CS_OK;
}

extern "C" int cs_merge_constraints_header_get(cs_merge_constraints* mc, void* hip_stream, cs_merge_constraints_header* h_out) {
    if (!mc || !h_out) {
        cs_set_error("cs_merge_constraints_header_get: bad arguments");
        return CS_ERR_INVALID;
    }
    CS_HIP(hipSetDevice(mc->device));
    CS_HIP(hipMemcpyAsync(h_out, mc->b.header, sizeof(*h_out), hipMemcpyDeviceToHost, (hipStream_t)hip_stream));
    CS_HIP(hipStreamSynchronize((hipStream_t)hip_stream));
    return CS_OK;
}

extern "C" int cs_merge_constraints_download(cs_merge_constraints* mc, void* hip_stream, const void* d_src, void* h_dst, size_t bytes) {
    return cs_arena_download("cs_merge_constraints_download", mc ? mc->device : 0, mc ? mc->base : nullptr, mc ? mc->bytes : 0, hip_stream, d_src,
                             h_dst, bytes);
}

// ---- the two solves of :646-647: bundleAdjustRobust(1, ..., 1, ..., 800, 1, 100), then (..., 30, 5, 30) from the first one's result.
// The assembled problem is brought to the host and fed to the EXISTING robust BA through its host-pointer entry (cs_ba_robust_h ->
// cs_ba_upload), unchanged; a device-pointer upload would need more than copies.  Both results stay in the handle; the
// second one's poses, points and outlier flags go to the handle's own device buffers (solvedRs / solvedTs / solvedPts / outlier).
extern "C" int cs_merge_constraints_solve(cs_merge_constraints* mc, void* hip_stream) {
    const char* who = "cs_merge_constraints_solve";
    if (!mc) {
        cs_set_error("%s: bad arguments", who);
        return CS_ERR_INVALID;
    }
    hipStream_t s = (hipStream_t)hip_stream;
    mc->solved = 0;
    cs_merge_constraints_header h;
    int rc = cs_merge_constraints_header_get(mc, hip_stream, &h);
    if (rc) return rc;
    if (h.verdict != CS_MERGE_OK) return CS_OK;   // a rejected verdict: nothing to solve, cs_merge_constraints_info_dev gives nInfo = 0
    if (h.nPose < 2 || h.nPose > 32 || h.P < 1 || h.P > mc->maxPoints || h.nObs < 1 || h.nObs > mc->maxObs) {
        mc->solved = -1;
        cs_set_error("%s: the assembled problem has %d poses, %d points, %d measurements", who, h.nPose, h.P, h.nObs);
        return CS_ERR_INVALID;
    }
    const int C = h.nPose, P = h.P, nObs = h.nObs;
    const cs_merge_constraints_buffers& B = mc->b;
    mc->sC = C, mc->sP = P, mc->sObs = nObs;
    mc->hK.resize(9 * (size_t)C), mc->hXY.resize(2 * (size_t)nObs), mc->hPtr.resize((size_t)P + 1), mc->hCam.resize(nObs);
    for (int k = 0; k < 2; ++k) mc->hR[k].resize(9 * (size_t)C), mc->hT[k].resize(3 * (size_t)C), mc->hM[k].resize(3 * (size_t)P), mc->hOut[k].assign(nObs, 0);
    CS_HIP(hipMemcpyAsync(mc->hK.data(), B.Ks, 72 * (size_t)C, hipMemcpyDeviceToHost, s));
    CS_HIP(hipMemcpyAsync(mc->hR[0].data(), B.Rs, 72 * (size_t)C, hipMemcpyDeviceToHost, s));
    CS_HIP(hipMemcpyAsync(mc->hT[0].data(), B.Ts, 24 * (size_t)C, hipMemcpyDeviceToHost, s));
    CS_HIP(hipMemcpyAsync(mc->hM[0].data(), B.pts, 24 * (size_t)P, hipMemcpyDeviceToHost, s));
    CS_HIP(hipMemcpyAsync(mc->hPtr.data(), B.obsPtr, 4 * ((size_t)P + 1), hipMemcpyDeviceToHost, s));
    CS_HIP(hipMemcpyAsync(mc->hCam.data(), B.obsCam, 4 * (size_t)nObs, hipMemcpyDeviceToHost, s));
    CS_HIP(hipMemcpyAsync(mc->hXY.data(), B.obsXY, 16 * (size_t)nObs, hipMemcpyDeviceToHost, s));
    CS_HIP(hipStreamSynchronize(s));
    if (!mc->ba) mc->ba = cs_ba_create(mc->device);
    if (!mc->ba) {
        mc->solved = -1;
        return CS_ERR_HIP;
    }
    static const double maxErr[2] = {800, 30};
    static const int maxIter[2] = {1, 5}, inner[2] = {100, 30};
    for (int k = 0; k < 2; ++k) {
        if (k) mc->hR[1] = mc->hR[0], mc->hT[1] = mc->hT[0], mc->hM[1] = mc->hM[0];   // the second solve starts from the first one's result
        rc = cs_ba_robust_h(mc->ba, C, P, nObs, mc->hK.data(), mc->hR[k].data(), mc->hT[k].data(), mc->hM[k].data(), mc->hPtr.data(), mc->hCam.data(),
                            mc->hXY.data(), 1, 1, maxErr[k], maxIter[k], inner[k], mc->hOut[k].data(), &mc->stats[k]);
        if (rc) {   // a failed solve touches nothing: the device buffers keep what they held, info gives nInfo = 0
            mc->solved = -1;
            return rc;
        }
    }
    CS_HIP(hipSetDevice(mc->device));
    CS_HIP(hipMemcpyAsync((void*)B.solvedRs, mc->hR[1].data(), 72 * (size_t)C, hipMemcpyHostToDevice, s));
    CS_HIP(hipMemcpyAsync((void*)B.solvedTs, mc->hT[1].data(), 24 * (size_t)C, hipMemcpyHostToDevice, s));
    CS_HIP(hipMemcpyAsync((void*)B.solvedPts, mc->hM[1].data(), 24 * (size_t)P, hipMemcpyHostToDevice, s));
    CS_HIP(hipMemcpyAsync((void*)B.outlier, mc->hOut[1].data(), 4 * (size_t)nObs, hipMemcpyHostToDevice, s));
    CS_HIP(hipStreamSynchronize(s));   // (the host vectors may be resized by the next solve)
    mc->solved = 1;
    return CS_OK;
}

// solve `which` (0: maxErr 800, 1 x 100; 1: maxErr 30, 5 x 30) of the last cs_merge_constraints_solve, host copies; any pointer may be NULL
extern "C" int cs_merge_constraints_solution(const cs_merge_constraints* mc, int which, double* Rs, double* Ts, double* pts, int* outlier,
                                             cs_ba_stats* stats) {
    if (!mc || which < 0 || which > 1 || mc->solved != 1) {
        cs_set_error("cs_merge_constraints_solution: no successful solve to read (which = %d)", which);
        return CS_ERR_INVALID;
    }
    if (Rs) memcpy(Rs, mc->hR[which].data(), 72 * (size_t)mc->sC);
    if (Ts) memcpy(Ts, mc->hT[which].data(), 24 * (size_t)mc->sC);
    if (pts) memcpy(pts, mc->hM[which].data(), 24 * (size_t)mc->sP);
    if (outlier) memcpy(outlier, mc->hOut[which].data(), 4 * (size_t)mc->sObs);
    if (stats) *stats = mc->stats[which];
    return CS_OK;
}

// the MergeInfo list from the SOLVED poses; nInfo = 0 and nothing else written unless the verdict was CS_MERGE_OK and both solves succeeded
extern "C" int cs_merge_constraints_info_dev(cs_merge_constraints* mc, void* hip_stream, const cs_camera_groups* d_groups, int gId1, int gId2) {
    if (!mc || !d_groups) {
        cs_set_error("cs_merge_constraints_info_dev: bad arguments");
        return CS_ERR_INVALID;
    }
    if (mc->solved == 1) return cs_merge_info_dev(mc, hip_stream, d_groups, gId1, gId2, mc->b.solvedRs, mc->b.solvedTs);
    CS_HIP(hipSetDevice(mc->device));
    CS_HIP(hipMemsetAsync((char*)mc->b.header + offsetof(cs_merge_constraints_header, nInfo), 0, sizeof(int), (hipStream_t)hip_stream));
    return CS_OK;
}

// the merge list and the solved coordinates onto the live map tables: one launch of one workgroup, no host wait
extern "C" int cs_merge_constraints_apply_map_dev(cs_merge_constraints* mc, void* hip_stream, int* const* d_slot2map, int* d_pointFeat,
                                                  cs_feat_ref* d_featRef, unsigned char* d_refStatic, int nMap, double* d_mapPts, int applyPoints,
                                                  int* d_counts) {
    const char* who = "cs_merge_constraints_apply_map_dev";
    if (!mc || !d_slot2map || !d_featRef || nMap < 0) {
        cs_set_error("%s: null handle, slot2map list or feature references (nMap %d)", who, nMap);
        return CS_ERR_INVALID;
    }
    if (nMap > mc->maxMap) {
        cs_set_error("%s: %d map rows, the handle was created for %d", who, nMap, mc->maxMap);
        return CS_ERR_INVALID;
    }
    MmArgs A;
    memset(&A, 0, sizeof(A));
    for (int c = 0; c < mc->nCams; ++c) {
        if (!d_slot2map[c]) {
            cs_set_error("%s: null slot2map of camera %d", who, c);
            return CS_ERR_INVALID;
        }
        A.slot2map[c] = d_slot2map[c];
    }
    A.nCams = mc->nCams, A.N = mc->N, A.nMap = nMap, A.maxViews = mc->maxViews, A.maxPoints = mc->maxPoints;
    A.applyPts = applyPoints && d_mapPts && mc->solved == 1 ? 1 : 0;   // the reference merges before it solves: the list goes in either way
    A.hdr = mc->b.header, A.views = mc->b.views, A.pointMap = mc->b.pointMap, A.solvedPts = mc->b.solvedPts;
    A.pointFeat = d_pointFeat, A.featRef = (int4*)d_featRef, A.refStatic = d_refStatic, A.mapPts = d_mapPts, A.counts = d_counts;
    A.winSlot = mc->winSlot, A.winRow = mc->winRow, A.winPt = mc->winPt, A.gRef = mc->gRef, A.gStat = mc->gStat;
    CS_HIP(hipSetDevice(mc->device));
    hipLaunchKernelGGL(k_merge_apply_map, dim3(1), dim3(MC_T), 0, (hipStream_t)hip_stream, A);
    CS_CHECK_LAUNCH();
    return CS_OK;
}
