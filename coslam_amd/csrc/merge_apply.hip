// merge_apply.hip -- what a camera-group merge does to the map behind its pose correction, DESIGN 3.21.
//
// Replaces CoSLAM::getMapPts(fStart, fEnd) (src/app/SL_CoSLAM.cpp:1818-1851) followed by MergeCameraGroup::recomputeMapPoints
// (src/app/SL_MergeCameraGroup.cpp:1175-1183): every certain-static map point of the merged span is triangulated again by
// updateStaticPointPositionAtKeyFrms (src/slam/SL_CoSLAMHelper.cpp:395-451) from its KEY-FRAME views.  That function is not
// updateStaticPointPosition with a flag: a camera contributes only when the point's head feature in that camera is itself a key-frame
// feature (:402), the backward walk looks at key-frame nodes only (:423) and it has no length limit (:422) -- a merge spans up to 101
// key frames, many hundred frames of the store, where every walk of poseupdate.hip ends after histLen nodes of a centre table.
//
// A WAVE = one map point, as k_update_points.  A run of consecutive frames [lo, hi] of a chain maps to a slice of the ascending
// key-frame list by two binary searches; the lanes take 64 key frames of the slice at a time, newest first, each lane the camera centre
// from the history's R, t of that frame and the COSINE of the angle at the point's current M (acos is monotone; no libm on the device),
// and keep their first minimum; one fold at the end of the walk takes the smallest cosine, among equals the one that came first in the
// walk (a running node number carries the order across 64-blocks and across segments).  The cost of a walk scales with key frames, not
// frames; the only dependent chain is the segment hops, one int4 {slot, last, first, next} each.  The normal equations are summed view
// by view in the reference's order by every lane, the covariance as in k_update_points (lane c owns camera c's Jacobians).
//
// The second half of the file (cs_merge_apply_*) carries the pose correction of DESIGN 3.20 into the history behind a device-side guard.
#include <vector>

#include "cs_common.h"
#include "dev_arena.h"
#include "project_dev.h"
#include "triangulate_dev.h"
#include "history_view.h"
#include "posegraph_view.h"

namespace {

constexpr int RK_MAX_CAMS = 16;

struct RkArgs {
    int nCams, N, H, head, stored, curFrame;   // the history's ring: capacity, newest slot, frames held, the newest frame's number
    int nMap, fStart, fEnd, nKey, segCap, updateCov;
    const int* mapCount;             // [1] or null (= nMap)
    const int* firstFrame;           // [nMap]
    const int* lastFrame;            // [nMap]
    const unsigned char* mapFlags;   // [nMap]
    const int* keyFrames;            // [nKey] ascending
    const int4* featRef;             // [nMap][nCams] {slot, frame, first, seg}
    const int4* segPool;             // [nCams][segCap] {slot, last, first, next}
    const double *histXY, *histR, *histT;
    double* mapPts;
    double* mapCov;
    double sigma;
    int* counts;   // [4] or null: rows selected, re-triangulated, left with fewer than two views, walks cut
    const int* guard;   // or null; *guard != 0: nothing is done (cs_merge_apply_run_dev's solves failed)
    const double* K[RK_MAX_CAMS];
    const double* iK[RK_MAX_CAMS];
};

// the first index of keys[0 .. n) whose entry is >= f (n: none)
__device__ __forceinline__ int rk_lower_bound(const int* __restrict__ keys, int n, int f) {
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (keys[mid] < f) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// one map point, one wave (lane r): every test is uniform over the wave
__device__ __forceinline__ void rk_point(const RkArgs& A, int m, int r) {
    if (A.guard && *A.guard != 0) return;
    int mapCount = A.mapCount ? *A.mapCount : A.nMap;
    if (mapCount > A.nMap) mapCount = A.nMap;
    if (m >= mapCount) return;
    if (A.mapFlags[m] != 0 || A.lastFrame[m] < A.fStart || A.firstFrame[m] > A.fEnd) return;   // SL_CoSLAM.cpp:1827-1831
    const int N = A.N, H = A.H;
    const int oldest = A.curFrame - A.stored + 1;   // the oldest frame the store holds
    double M[3];
#pragma unroll
    for (int q = 0; q < 3; ++q) M[q] = A.mapPts[3 * (size_t)m + q];
    UpNormalEq E;
#pragma unroll
    for (int q = 0; q < 6; ++q) E.N[q] = 0;
#pragma unroll
    for (int q = 0; q < 3; ++q) E.g[q] = 0;
    int numView = 0, nCut = 0;
    int mySecond = -2, myFirst = 0;   // lane r keeps camera r's views as ring depths; second -1 none, -2 the camera gives nothing
    for (int c = 0; c < A.nCams; ++c) {
        const int4 ref = A.featRef[(size_t)m * A.nCams + c];
        const int s = ref.x, f0 = ref.y;
        if (s < 0 || s >= N || f0 < oldest || f0 > A.curFrame) continue;   // no feature, or one the store does not hold
        const int k0i = rk_lower_bound(A.keyFrames, A.nKey, f0);
        if (k0i >= A.nKey || A.keyFrames[k0i] != f0) continue;             // :402 the head is no key-frame feature: the camera gives nothing
        const double* hR = A.histR + (size_t)c * H * 9;
        const double* hT = A.histT + (size_t)c * H * 3;
        const double* hXY = A.histXY + (size_t)c * H * 2 * N;
        const int j0 = A.curFrame - f0, rs0 = (A.head - j0 + H) % H;
        const double* R0 = hR + (size_t)rs0 * 9;
        const double* t0 = hT + (size_t)rs0 * 3;
        up_add_view(E, A.iK[c], R0, t0, hXY[(size_t)rs0 * 2 * N + s], hXY[(size_t)rs0 * 2 * N + N + s]);   // :407-414
        ++numView;
        double C0[3];
        up_cam_center(R0, t0, C0);
        const double a[3] = {C0[0] - M[0], C0[1] - M[1], C0[2] - M[2]};
        const double na = (a[0] * a[0] + a[1] * a[1]) + a[2] * a[2];
        // :419-433 fp = fp->preFrame ... while (fp): the whole chain, key-frame nodes only
        int best = -1, bestK = 0x7fffffff, bSlot = -1;
        double bestCos = 1.0;
        int slot = s, hi = f0 - 1, lo = ref.z, seg = ref.w, node = 0, hops = 0;
        for (;;) {
            const bool cut = lo < oldest;
            const int flo = cut ? oldest : lo, fhi = hi < A.curFrame ? hi : A.curFrame;
            if (fhi >= flo) {
                const int ka = rk_lower_bound(A.keyFrames, A.nKey, flo), kb = rk_lower_bound(A.keyFrames, A.nKey, fhi + 1);
                const int cnt = kb - ka;   // the key frames of [flo, fhi], walked newest first
                for (int i = r; i < cnt; i += 64) {
                    const int j = A.curFrame - A.keyFrames[kb - 1 - i];
                    const int rs = (A.head - j + H) % H;
                    double Cj[3];
                    up_cam_center(hR + (size_t)rs * 9, hT + (size_t)rs * 3, Cj);
                    const double b0 = Cj[0] - M[0], b1 = Cj[1] - M[1], b2 = Cj[2] - M[2];
                    const double d = (a[0] * b0 + a[1] * b1) + a[2] * b2;
                    const double nb = (b0 * b0 + b1 * b1) + b2 * b2;
                    const double cv = d / sqrt(na * nb);
                    if (cv < bestCos) bestCos = cv, best = j, bestK = node + i, bSlot = slot;   // (i ascending: the first of equal cosines stays)
                }
                node += cnt;
            }
            if (cut) {   // the chain goes on behind the store's oldest frame: those nodes are no views
                ++nCut;
                break;
            }
            if (seg < 0) break;
            if (seg >= A.segCap || hops >= A.segCap) {   // a corrupt pool: an index outside it, or more hops than it has segments
                ++nCut;
                break;
            }
            const int4 g = A.segPool[(size_t)c * A.segCap + seg];
            ++hops;
            if (g.x < 0 || g.x >= N) {   // (a segment of no slot: corrupt as well)
                ++nCut;
                break;
            }
            slot = g.x, hi = g.y, lo = g.z, seg = g.w;
        }
        for (int off = 1; off < 64; off <<= 1) {
            const double oc = __shfl_xor(bestCos, off, 64);
            const int oj = __shfl_xor(best, off, 64), ok = __shfl_xor(bestK, off, 64), os = __shfl_xor(bSlot, off, 64);
            if (oj >= 0 && (oc < bestCos || (oc == bestCos && ok < bestK))) bestCos = oc, best = oj, bestK = ok, bSlot = os;
        }
        if (best >= 0) {   // :434-443
            const int rs = (A.head - best + H) % H;
            up_add_view(E, A.iK[c], hR + (size_t)rs * 9, hT + (size_t)rs * 3, hXY[(size_t)rs * 2 * N + bSlot], hXY[(size_t)rs * 2 * N + N + bSlot]);
            ++numView;
        }
        if (r == c) mySecond = best, myFirst = j0;
    }
    if (r == 0 && A.counts) {
        atomicAdd(A.counts + 0, 1);
        atomicAdd(A.counts + (numView >= 2 ? 1 : 2), 1);
        if (nCut) atomicAdd(A.counts + 3, nCut);
    }
    if (numView < 2) return;   // :446
    double cf[6];
    const double det = up_sym33_cof(E.N, cf);
    M[0] = ((cf[0] * E.g[0] + cf[1] * E.g[1]) + cf[2] * E.g[2]) / det;   // triangulateMultiView
    M[1] = ((cf[1] * E.g[0] + cf[3] * E.g[1]) + cf[4] * E.g[2]) / det;
    M[2] = ((cf[2] * E.g[0] + cf[4] * E.g[1]) + cf[5] * E.g[2]) / det;
    if (A.updateCov) {   // getTriangulateCovMat at the new point: lane c computes camera c's Jacobians, every lane sums them in view order
        double J1[6] = {0, 0, 0, 0, 0, 0}, J2[6] = {0, 0, 0, 0, 0, 0};
        if (r < A.nCams && mySecond != -2) {
            const double* hR = A.histR + (size_t)r * H * 9;
            const double* hT = A.histT + (size_t)r * H * 3;
            const int rs1 = (A.head - myFirst + H) % H;
            const PuProj q1 = pu_project(A.K[r], hR + (size_t)rs1 * 9, hT + (size_t)rs1 * 3, M);
#pragma unroll
            for (int k = 0; k < 6; ++k) J1[k] = q1.J[k];
            if (mySecond >= 0) {
                const int rs = (A.head - mySecond + H) % H;
                const PuProj q2 = pu_project(A.K[r], hR + (size_t)rs * 9, hT + (size_t)rs * 3, M);
#pragma unroll
                for (int k = 0; k < 6; ++k) J2[k] = q2.J[k];
            }
        }
        double S[6] = {0, 0, 0, 0, 0, 0};
        for (int c = 0; c < A.nCams; ++c) {
            const int sv = __shfl(mySecond, c, 64);
            if (sv == -2) continue;
            double Jc[6];
#pragma unroll
            for (int k = 0; k < 6; ++k) Jc[k] = __shfl(J1[k], c, 64);
            up_add_jtj(S, Jc);
            if (sv >= 0) {
#pragma unroll
                for (int k = 0; k < 6; ++k) Jc[k] = __shfl(J2[k], c, 64);
                up_add_jtj(S, Jc);
            }
        }
        if (r == 0) {
            const double dS = up_sym33_cof(S, cf), s2 = A.sigma * A.sigma;
            double* cov = A.mapCov + 9 * (size_t)m;
            const double c01 = (cf[1] / dS) * s2, c02 = (cf[2] / dS) * s2, c12 = (cf[4] / dS) * s2;
            cov[0] = (cf[0] / dS) * s2, cov[1] = c01, cov[2] = c02;
            cov[3] = c01, cov[4] = (cf[3] / dS) * s2, cov[5] = c12;
            cov[6] = c02, cov[7] = c12, cov[8] = (cf[5] / dS) * s2;
        }
    }
    if (r != 0) return;
#pragma unroll
    for (int q = 0; q < 3; ++q) A.mapPts[3 * (size_t)m + q] = M[q];
}

__global__ __launch_bounds__(256) void k_recompute_keyfrms(RkArgs A) {
    const int tid = threadIdx.x, g = tid / 64, r = tid % 64;
    rk_point(A, blockIdx.x * 4 + g, r);
}

}  // namespace

extern "C" int cs_recompute_map_points_keyfrms_dev(const cs_track_history* h, void* hip_stream, const cs_poseupdate_cam* cams,
                                                   const cs_feat_ref* d_featRef, int nMap, const int* d_mapCount, const int* d_firstFrame,
                                                   const int* d_lastFrame, const unsigned char* d_mapFlags, int fStart, int fEnd,
                                                   const int* d_keyFrames, int nKey, double* d_mapPts, double* d_mapCov, double pixelErrVar,
                                                   int updateCov, int* d_counts, const int* d_guard) {
    const char* who = "cs_recompute_map_points_keyfrms_dev";
    if (!h || !cams || !d_featRef || nMap < 0 || !d_firstFrame || !d_lastFrame || !d_mapFlags || nKey < 0 || (nKey > 0 && !d_keyFrames) ||
        !d_mapPts || (updateCov && !d_mapCov)) {
        cs_set_error("%s: bad arguments", who);
        return CS_ERR_INVALID;
    }
    CsHistView v;
    cs_history_view(h, &v);
    if (v.stored < 1) {
        cs_set_error("%s: the history holds no frame", who);
        return CS_ERR_INVALID;
    }
    if (v.nCams > RK_MAX_CAMS) {
        cs_set_error("%s: at most %d cameras", who, RK_MAX_CAMS);
        return CS_ERR_INVALID;
    }
    RkArgs A;
    A.nCams = v.nCams, A.N = v.N, A.H = v.H, A.head = v.head, A.stored = v.stored, A.curFrame = v.lastFrame;
    A.nMap = nMap, A.fStart = fStart, A.fEnd = fEnd, A.nKey = nKey, A.segCap = v.segCap, A.updateCov = updateCov ? 1 : 0;
    A.mapCount = d_mapCount, A.firstFrame = d_firstFrame, A.lastFrame = d_lastFrame, A.mapFlags = d_mapFlags, A.keyFrames = d_keyFrames;
    A.featRef = (const int4*)d_featRef, A.segPool = v.segPool;
    A.histXY = v.xy, A.histR = v.R, A.histT = v.t;
    A.mapPts = d_mapPts, A.mapCov = d_mapCov, A.sigma = pixelErrVar, A.counts = d_counts, A.guard = d_guard;
    for (int c = 0; c < RK_MAX_CAMS; ++c) A.K[c] = A.iK[c] = nullptr;
    for (int c = 0; c < v.nCams; ++c) {
        if (!cams[c].K || !cams[c].iK) {
            cs_set_error("%s: null K / iK in camera %d", who, c);
            return CS_ERR_INVALID;
        }
        A.K[c] = cams[c].K, A.iK[c] = cams[c].iK;
    }
    if (nMap == 0) return CS_OK;
    CS_HIP(hipSetDevice(v.device));
    hipLaunchKernelGGL(k_recompute_keyfrms, dim3((nMap + 3) / 4), dim3(256), 0, (hipStream_t)hip_stream, A);
    CS_HIP(hipGetLastError());
    return CS_OK;
}

// ---- the corrected poses into the history: MergeCameraGroup::recomputeKeyCamPoses + recomputeAllCameraPoses
// (src/app/SL_MergeCameraGroup.cpp:1083-1116) fed from and written to a cs_track_history, no host wait ---------------------------------
// The chain graphs of _constructGraphForAllFrms (:1037-1082) for ALL cameras: one node per frame of [keyFrames[0], keyFrames[nKey - 1]],
// fixed at the key frames, one edge per consecutive pair -- flat node (c, f) = c * nFrames + (f - keyFrames[0]), which is the layout of
// cs_track_history_get_span_dev, so the span is read straight into the chains' node arrays and written back from their result.

namespace {

// rows src[idx[i]] of [.][9] / [.][3] arrays into row i (gather) or row i into dst[idx[i]] (scatter); idx < 0: skipped
__global__ __launch_bounds__(128) void k_merge_rows(int n, const int* __restrict__ idx, int scatter, const double* __restrict__ srcR,
                                                    const double* __restrict__ srcT, double* dstR, double* dstT) {
    const int q = blockIdx.x * 128 + threadIdx.x, i = q / 12, e = q - 12 * i;
    if (i >= n) return;
    const int j = idx[i];
    if (j < 0) return;
    const size_t from = scatter ? (size_t)i : (size_t)j, to = scatter ? (size_t)j : (size_t)i;
    if (e < 9)
        dstR[9 * to + e] = srcR[9 * from + e];
    else
        dstT[3 * to + (e - 9)] = srcT[3 * from + (e - 9)];
}

// *guard = any status word of the two solves is non-zero
__global__ __launch_bounds__(64) void k_merge_guard(const int* __restrict__ st1, int n1, const int* __restrict__ st2, int n2, int* guard) {
    int bad = 0;
    for (int i = threadIdx.x; i < n1; i += 64) bad |= st1[i] != 0;
    for (int i = threadIdx.x; i < n2; i += 64) bad |= st2[i] != 0;
    const unsigned long long any = __ballot(bad);
    if (threadIdx.x == 0) *guard = any ? 1 : 0;
}

}  // namespace

struct cs_merge_apply {
    int device = 0, nCams = 0, nKey = 0, firstFrame = 0, lastFrame = 0, nFrames = 0;
    int nKeyNodes = 0, nKeyEdges = 0, nChainNodes = 0, nChainEdges = 0, nConstraint = 0;
    cs_posegraph *key = nullptr, *chains = nullptr;
    char* dev = nullptr;   // one allocation: the arrays below
    int *keyNode = nullptr, *conRow = nullptr, *guard = nullptr, *keyFrames = nullptr;
    double *kR, *kT, *keR, *keT, *knR, *knT, *keS, *cR, *cT, *ceR, *ceT, *cnR, *cnT;
};

extern "C" void cs_merge_apply_destroy(cs_merge_apply* a) {
    if (!a) return;
    (void)hipSetDevice(a->device);
    if (a->key) cs_posegraph_destroy(a->key);
    if (a->chains) cs_posegraph_destroy(a->chains);
    if (a->dev) (void)hipFree(a->dev);
    delete a;
}

extern "C" cs_merge_apply* cs_merge_apply_create(int device, int nCams, int nKey, const int* keyFrames, int nNodes, const int* nodeKf,
                                                 const int* nodeCam, const unsigned char* fixed, int nEdges, const int* id1, const int* id2,
                                                 const int* scaleId) {
    const char* who = "cs_merge_apply_create";
    if (nCams < 1 || nCams > RK_MAX_CAMS || nKey < 2 || !keyFrames || nNodes < 1 || !nodeKf || !nodeCam || !fixed || nEdges < 0 ||
        (nEdges > 0 && (!id1 || !id2 || !scaleId))) {
        cs_set_error("%s: bad arguments (1..%d cameras, at least two key frames)", who, RK_MAX_CAMS);
        return nullptr;
    }
    for (int k = 1; k < nKey; ++k)
        if (keyFrames[k] <= keyFrames[k - 1]) {
            cs_set_error("%s: key frames must be ascending", who);
            return nullptr;
        }
    const long long nF64 = (long long)keyFrames[nKey - 1] - keyFrames[0] + 1;
    if (nF64 > 65536) {
        cs_set_error("%s: a span of %lld frames is longer than any store", who, nF64);
        return nullptr;
    }
    const int nF = (int)nF64;
    std::vector<int> keyNode(nNodes), conRow;
    for (int i = 0; i < nNodes; ++i) {
        if (nodeKf[i] < 0 || nodeKf[i] >= nKey || nodeCam[i] < 0 || nodeCam[i] >= nCams) {
            cs_set_error("%s: node %d names key frame %d / camera %d", who, i, nodeKf[i], nodeCam[i]);
            return nullptr;
        }
        keyNode[i] = nodeCam[i] * nF + (keyFrames[nodeKf[i]] - keyFrames[0]);
    }
    for (int e = 0; e < nEdges; ++e)
        if (scaleId[e] >= 0) conRow.push_back(e);
    // _constructGraphForAllFrms, every camera
    std::vector<unsigned char> cFixed((size_t)nCams * nF, 0);
    std::vector<int> cId1((size_t)nCams * (nF - 1)), cId2((size_t)nCams * (nF - 1)), nodePtr(nCams + 1), edgePtr(nCams + 1);
    for (int c = 0; c <= nCams; ++c) nodePtr[c] = c * nF, edgePtr[c] = c * (nF - 1);
    for (int c = 0; c < nCams; ++c) {
        for (int k = 0; k < nKey; ++k) cFixed[(size_t)c * nF + (keyFrames[k] - keyFrames[0])] = 1;
        for (int i = 0; i + 1 < nF; ++i) cId1[(size_t)c * (nF - 1) + i] = i, cId2[(size_t)c * (nF - 1) + i] = i + 1;
    }
    if (hipSetDevice(device) != hipSuccess) {
        cs_set_error("%s: no usable HIP device %d (there is no CPU fallback)", who, device);
        return nullptr;
    }
    cs_merge_apply* a = new cs_merge_apply();
    a->device = device, a->nCams = nCams, a->nKey = nKey, a->firstFrame = keyFrames[0], a->lastFrame = keyFrames[nKey - 1], a->nFrames = nF;
    a->nKeyNodes = nNodes, a->nKeyEdges = nEdges, a->nChainNodes = nCams * nF, a->nChainEdges = nCams * (nF - 1);
    a->nConstraint = (int)conRow.size();
    const int kNodePtr[2] = {0, nNodes}, kEdgePtr[2] = {0, nEdges};
    if (cs_posegraph_create_scaled(device, 1, kNodePtr, kEdgePtr, fixed, id1, id2, scaleId, &a->key) != CS_OK ||
        cs_posegraph_create(device, nCams, nodePtr.data(), edgePtr.data(), cFixed.data(), cId1.data(), cId2.data(), &a->chains) != CS_OK) {
        cs_merge_apply_destroy(a);   // (cs_last_error: the pose graph's)
        return nullptr;
    }
    const size_t nk = nNodes, ek = nEdges > 0 ? nEdges : 1, nc = a->nChainNodes, ec = a->nChainEdges > 0 ? a->nChainEdges : 1;
    size_t bytes;
    const bool ok = cs_arena_alloc(device, a->dev, bytes, [&](CsArena& ar) {
        ar.take(a->kR, 9 * nk), ar.take(a->kT, 3 * nk), ar.take(a->knR, 9 * nk), ar.take(a->knT, 3 * nk);
        ar.take(a->keR, 9 * ek), ar.take(a->keT, 3 * ek), ar.take(a->keS, ek);
        ar.take(a->cR, 9 * nc), ar.take(a->cT, 3 * nc), ar.take(a->cnR, 9 * nc), ar.take(a->cnT, 3 * nc);
        ar.take(a->ceR, 9 * ec), ar.take(a->ceT, 3 * ec);
        ar.take(a->keyNode, nk), ar.take(a->conRow, ek), ar.take(a->guard, 2), ar.take(a->keyFrames, nKey);
    });
    if (!ok) {
        cs_set_error("%s: hipMalloc failed", who);
        cs_merge_apply_destroy(a);
        return nullptr;
    }
    if (hipMemcpy(a->keyNode, keyNode.data(), 4 * nk, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(a->keyFrames, keyFrames, 4 * (size_t)nKey, hipMemcpyHostToDevice) != hipSuccess ||
        (!conRow.empty() && hipMemcpy(a->conRow, conRow.data(), 4 * conRow.size(), hipMemcpyHostToDevice) != hipSuccess)) {
        cs_set_error("%s: upload failed", who);
        cs_merge_apply_destroy(a);
        return nullptr;
    }
    return a;
}

extern "C" const int* cs_merge_apply_guard(const cs_merge_apply* a) { return a ? a->guard : nullptr; }
extern "C" const int* cs_merge_apply_key_frames(const cs_merge_apply* a, int* nKey) {
    if (nKey) *nKey = a ? a->nKey : 0;
    return a ? a->keyFrames : nullptr;
}

extern "C" int cs_merge_apply_run_dev(cs_merge_apply* a, cs_track_history* h, void* hip_stream, const double* d_infoR, const double* d_infoT,
                                      double* d_edgeS) {
    const char* who = "cs_merge_apply_run_dev";
    if (!a || !h || (a->nConstraint > 0 && (!d_infoR || !d_infoT))) {
        cs_set_error("%s: bad arguments", who);
        return CS_ERR_INVALID;
    }
    CsHistView v;
    cs_history_view(h, &v);
    if (v.nCams != a->nCams || v.device != a->device) {
        cs_set_error("%s: the history has %d camera(s) on device %d, the handle was built for %d on device %d", who, v.nCams, v.device, a->nCams,
                     a->device);
        return CS_ERR_INVALID;
    }
    if (v.stored < 1 || v.lastFrame != a->lastFrame) {
        cs_set_error("%s: the history's newest frame is %d, not the current key frame %d", who, v.stored < 1 ? -1 : v.lastFrame, a->lastFrame);
        return CS_ERR_INVALID;
    }
    if (v.lastFrame - a->firstFrame >= v.stored) {
        cs_set_error("%s: the fixed key frame %d has left the store (it holds frames %d..%d): an archived pose is final", who, a->firstFrame,
                     v.lastFrame - v.stored + 1, v.lastFrame);
        return CS_ERR_INVALID;
    }
    hipStream_t s = (hipStream_t)hip_stream;
    int rc;
    CS_HIP(hipSetDevice(a->device));
    // 1. the span  2. the key nodes  3. plain key edges and all chain edges from the poses BEFORE the correction (constructGraphForAllFrms
    // runs before recomputeKeyCamPoses)  4. the constraint rows
    if ((rc = cs_track_history_get_span_dev(h, hip_stream, a->firstFrame, a->nFrames, a->cR, a->cT))) return rc;
    hipLaunchKernelGGL(k_merge_rows, dim3((a->nKeyNodes * 12 + 127) / 128), dim3(128), 0, s, a->nKeyNodes, a->keyNode, 0, a->cR, a->cT, a->kR,
                       a->kT);
    CS_CHECK_LAUNCH();
    if ((rc = cs_posegraph_edges_dev(a->key, hip_stream, a->kR, a->kT, a->keR, a->keT))) return rc;
    if ((rc = cs_posegraph_edges_dev(a->chains, hip_stream, a->cR, a->cT, a->ceR, a->ceT))) return rc;
    if (a->nConstraint > 0) {
        hipLaunchKernelGGL(k_merge_rows, dim3((a->nConstraint * 12 + 127) / 128), dim3(128), 0, s, a->nConstraint, a->conRow, 1, d_infoR, d_infoT,
                           a->keR, a->keT);
        CS_CHECK_LAUNCH();
    }
    // 5. the key graph  6. its poses into the chains' fixed nodes  7. the chains
    if ((rc = cs_posegraph_relax_scaled_dev(a->key, hip_stream, a->kR, a->kT, a->keR, a->keT, a->knR, a->knT, a->keS))) return rc;
    if ((rc = cs_posegraph_set_poses_dev(a->device, hip_stream, a->nKeyNodes, a->keyNode, a->knR, a->knT, a->cR, a->cT))) return rc;
    if ((rc = cs_posegraph_relax_dev(a->chains, hip_stream, a->cR, a->cT, a->ceR, a->ceT, a->cnR, a->cnT))) return rc;
    // 8. the write-back, behind the solves' status words read on the device
    const int *st1, *st2;
    int n1, n2;
    cs_posegraph_status_words(a->key, &st1, &n1);
    cs_posegraph_status_words(a->chains, &st2, &n2);
    hipLaunchKernelGGL(k_merge_guard, dim3(1), dim3(64), 0, s, st1, n1, st2, n2, a->guard);
    CS_CHECK_LAUNCH();
    if ((rc = cs_track_history_set_span_guarded_dev(h, hip_stream, a->firstFrame, a->nFrames, a->cnR, a->cnT, a->guard))) return rc;
    if (d_edgeS && a->nKeyEdges > 0) CS_HIP(hipMemcpyAsync(d_edgeS, a->keS, 8 * (size_t)a->nKeyEdges, hipMemcpyDeviceToDevice, s));
    return CS_OK;
}

extern "C" int cs_merge_apply_status(cs_merge_apply* a, void* hip_stream) {
    if (!a) {
        cs_set_error("cs_merge_apply_status: null handle");
        return CS_ERR_INVALID;
    }
    int nFailed = 0, first = -1;
    int rc = cs_posegraph_status(a->key, hip_stream, &nFailed, &first);
    if (rc == CS_ERR_NUMERIC) {
        cs_set_error("cs_merge_apply_status: the key-frame graph failed (%d component(s)): nothing was written", nFailed);
        return rc;
    }
    if (rc != CS_OK) return rc;
    rc = cs_posegraph_status(a->chains, hip_stream, &nFailed, &first);
    if (rc == CS_ERR_NUMERIC) cs_set_error("cs_merge_apply_status: the chain of camera %d failed (%d in all): nothing was written", first, nFailed);
    return rc;
}
