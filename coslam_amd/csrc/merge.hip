// merge.hip -- MergeCameraGroup::checkPossibleMergable per key frame, on the device (gfx950, wave64).
//
// Replaces the front half of CoSLAM::mergeCamGroups (src/app/SL_CoSLAM.cpp:1375-1384): checkPossibleMergable / ...Between / checkCamDist /
// checkViewOverlapFromTo / checkViewOverlap (src/app/SL_MergeCameraGroup.cpp:56-177) over the key frame's record of the camera groups
// (KeyFrame::setCamGroups, src/slam/SL_KeyPoseList.h:134-139): which camera pairs of two SEPARATED groups look at the same part of the map
// again and stand close enough.  It only reads state.  get2DConvexHull and poly2Mask are LibVisualSLAM functions that are not in the
// reference tree: the hull is hull_dev.h's (the one k_group_hull takes the area of), the mask is the CLOSED hull polygon -- the pixel
// (x, y) is set when the integer point gives <= 0 on every edge with the hull's own orientation function; a hull with fewer than three
// vertices sets no pixel.
//
// NOT BUILT HERE: what stands behind the gate.  Of it storeFeaturePoints and the front of matchMergableCameras (SURF, estimateEMat, the
// guided matcher) stay on the host; genMergeInfoVer2 up to and behind its solver call is merge_constraints.hip, the pose graphs
// posegraph.hip / merge_graph.cpp (3.20), mergeMatchedGroups and recomputeMapPoints merge_apply.hip (3.21).  The m_lastFrmGroupMerge + 130
// hold-off of mergeCamGroups (:1376) is the caller's: no loop merges yet, so m_lastFrmGroupMerge never moves and it could never fire.
//
// One launch: one workgroup per ORDERED camera pair (i, j).  It compacts camera i's features with a non-false map point in slot
// order, projects them with camera j's K, R, t (project_dev.h), keeps the in-image projections in LDS (nInCam), takes their hull when
// nInCam >= minInNum, and tests camera j's feature pixels, one per lane, against the hull's edges (inNum).  Integer counts by ballot and
// popcount only: two calls give the same bytes.  A workgroup whose cameras share a group leaves at once (unless allPairs), and with one
// group the whole launch does after one word per workgroup.  The workgroup whose ticket (an integer vector atomic on global memory) comes
// last forms fromTo, the centre distances and the MergeInfo list in the reference's loop order and leaves the scratch zeroed.
#include "cs_common.h"
#include "hull_dev.h"
#include "project_dev.h"

namespace {

constexpr int MG_MAX_CAMS = 16;
constexpr int MG_TAB = MG_MAX_CAMS * MG_MAX_CAMS;
constexpr int MG_THREADS = 1024;
constexpr int MG_MAX_INFO = 256;
constexpr size_t MG_MAX_LDS = 160u * 1024u - 1024u;   // a workgroup's LDS on gfx950, less the kernel's static words (as the grouping's hull)
// scratch (ints): [0, 256) nInCam + 1, [256, 512) inNum + 1, [512, 528) nFeat + 1 (0: nothing written), [528] ticket
constexpr int MG_SCR_IN = 0, MG_SCR_NUM = MG_TAB, MG_SCR_FEAT = 2 * MG_TAB, MG_SCR_TICKET = 2 * MG_TAB + MG_MAX_CAMS;
constexpr size_t MG_SCRATCH_BYTES = (MG_SCR_TICKET + 2) * sizeof(int);
constexpr int MG_G_WORDS = (int)(sizeof(cs_camera_groups) / sizeof(int));
constexpr int MG_INFO_WORDS = MG_MAX_INFO * 6;
// the finish's tables: camDist [256] doubles; nInCam, inNum [256], nFeat [16], the groups record, info[] as ints; fromTo [256] bytes
constexpr size_t MG_FINISH_LDS = MG_TAB * sizeof(double) + (2 * MG_TAB + MG_MAX_CAMS + MG_G_WORDS + MG_INFO_WORDS) * sizeof(int) + MG_TAB;

struct MgArgs {
    int nCams, N, nMap, W, H, frame, minInNum, allPairs;
    double ratio, maxCamDist;
    const int* mapCount;
    const double* mapPts;
    const unsigned char* mapFlags;
    const cs_camera_groups* groups;
    cs_merge_candidates* out;
    int* scratch;
    const double* xy[MG_MAX_CAMS];
    const int* state[MG_MAX_CAMS];
    const int* slot2map[MG_MAX_CAMS];
    const double* K[MG_MAX_CAMS];
    const double* R[MG_MAX_CAMS];
    const double* t[MG_MAX_CAMS];
};

// the map point of camera c's slot s when the slot is a feature of the key frame whose point takes part (SL_MergeCameraGroup.cpp:106-107,
// :153-154: fp->mpt && (isLocalStatic() || isLocalDynamic()), i.e. not false), or -1
__device__ __forceinline__ int mg_point(const MgArgs& A, int c, int s, int mapCount) {
    const int st = A.state[c][s];
    if (st != 0 && st != 1) return -1;
    const int m = A.slot2map[c][s];
    if (m < 0 || m >= mapCount) return -1;
    if (A.mapFlags && (A.mapFlags[m] & CS_MAP_FALSE)) return -1;
    return m;
}

// where this thread's flagged item goes among the workgroup's, in thread order, behind *sBase; *sBase moves on by the chunk's count
__device__ __forceinline__ int mg_place(bool flag, int* sWave, int* sBase) {
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const unsigned long long b = __builtin_amdgcn_ballot_w64(flag);
    if (lane == 0) sWave[wv] = __popcll(b);
    __syncthreads();
    int off = *sBase;
    for (int w = 0; w < wv; ++w) off += sWave[w];
    off += __popcll(b & ((1ull << lane) - 1ull));
    __syncthreads();
    if (tid == 0) {
        int tot = *sBase;
        for (int w = 0; w < MG_THREADS / 64; ++w) tot += sWave[w];
        *sBase = tot;
    }
    __syncthreads();
    return off;
}

// fromTo, checkCamDist and checkPossibleMergable's loops (:56-96, :166, :173-177): one workgroup, after every pair's counts have landed
__device__ void mg_finish(const MgArgs& A, double* sDyn) {
    double* sDist = sDyn;                         // [256]
    int* sIn = (int*)(sDist + MG_TAB);            // [256]
    int* sNum = sIn + MG_TAB;                     // [256]
    int* sFeat = sNum + MG_TAB;                   // [16]
    int* sG = sFeat + MG_MAX_CAMS;                // the cs_camera_groups record as ints
    int* sInfo = sG + MG_G_WORDS;                 // info[] as ints
    unsigned char* sFT = (unsigned char*)(sInfo + MG_INFO_WORDS);   // [256]
    __shared__ int sNInfo;
    const int tid = threadIdx.x, nC = A.nCams;
    constexpr int G_NUM = 1, G_IDS = 1 + MG_MAX_CAMS;
    if (tid < MG_TAB) {
        sIn[tid] = atomicExch(A.scratch + MG_SCR_IN + tid, 0) - 1;   // (the value in L2, and zero for the next call)
        sNum[tid] = atomicExch(A.scratch + MG_SCR_NUM + tid, 0) - 1;
    }
    if (tid < MG_MAX_CAMS) sFeat[tid] = atomicExch(A.scratch + MG_SCR_FEAT + tid, 0) - 1;
    for (int e = tid; e < MG_G_WORDS; e += MG_THREADS) sG[e] = ((const int*)A.groups)[e];
    for (int e = tid; e < MG_INFO_WORDS; e += MG_THREADS) sInfo[e] = -1;
    __syncthreads();
    if (tid < MG_TAB) {
        const int i = tid / MG_MAX_CAMS, j = tid % MG_MAX_CAMS;
        const int inNum = sNum[tid], totalNum = sFeat[j];
        const bool ft = inNum >= 0 && (inNum > 50 || (double)inNum >= A.ratio * (double)totalNum);   // :166
        double d = 0.0;
        if (i < nC && j < nC && i != j) {   // getCamCenter: -R^T t (:89-92)
            double Ci[3], Cj[3];
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                Ci[k] = -((A.R[i][k] * A.t[i][0] + A.R[i][3 + k] * A.t[i][1]) + A.R[i][6 + k] * A.t[i][2]);
                Cj[k] = -((A.R[j][k] * A.t[j][0] + A.R[j][3 + k] * A.t[j][1]) + A.R[j][6 + k] * A.t[j][2]);
            }
            const double dx = Ci[0] - Cj[0], dy = Ci[1] - Cj[1], dz = Ci[2] - Cj[2];
            d = sqrt((dx * dx + dy * dy) + dz * dz);
        }
        sFT[tid] = ft, sDist[tid] = d;
        A.out->nInCam[i][j] = sIn[tid], A.out->inNum[i][j] = inNum, A.out->fromTo[i][j] = ft, A.out->camDist[i][j] = d;
    }
    if (tid < MG_MAX_CAMS) A.out->nFeat[tid] = sFeat[tid];
    __syncthreads();
    if (tid == 0) {   // the reference's loop order (:59-64, :72-83); a record that names no camera of the rig is walked past
        const int gN = min(max(sG[0], 0), MG_MAX_CAMS);
        int n = 0;
        for (int g1 = 0; g1 < gN; ++g1)
            for (int g2 = g1 + 1; g2 < gN; ++g2) {
                const int n1 = min(max(sG[G_NUM + g1], 0), MG_MAX_CAMS), n2 = min(max(sG[G_NUM + g2], 0), MG_MAX_CAMS);
                for (int a = 0; a < n1; ++a) {
                    const int i = sG[G_IDS + g1 * MG_MAX_CAMS + a];
                    if (i < 0 || i >= nC) continue;
                    for (int b = 0; b < n2; ++b) {
                        const int j = sG[G_IDS + g2 * MG_MAX_CAMS + b];
                        if (j < 0 || j >= nC || j == i) continue;
                        const int e = i * MG_MAX_CAMS + j, r = j * MG_MAX_CAMS + i;
                        if (sFT[e] && sFT[r] && !(sDist[e] > A.maxCamDist) && n < MG_MAX_INFO) {   // :76-77, :93
                            int* q = sInfo + 6 * n++;
                            q[0] = A.frame, q[1] = i, q[2] = g1, q[3] = A.frame, q[4] = j, q[5] = g2;   // MergeInfo::set (:78-79)
                        }
                    }
                }
            }
        sNInfo = n;
    }
    __syncthreads();
    int* info = (int*)A.out->info;
    for (int e = tid; e < MG_INFO_WORDS; e += MG_THREADS) info[e] = sInfo[e];
    if (tid == 0) A.out->frame = A.frame, A.out->groupNum = sG[0], A.out->nMergeInfo = sNInfo, A.out->reserved = 0;
}

__global__ __launch_bounds__(MG_THREADS) void k_merge_check(MgArgs A, int cap) {
    extern __shared__ double sDyn[];
    // per point 32 bytes, as k_group_hull: xy, the best distance, the label, the best index (hull_dev.h)
    double* sXY = sDyn;                                                          // [cap][2]
    unsigned long long* sBestD = (unsigned long long*)(sXY + 2 * (size_t)cap);   // [cap]
    int* sLabel = (int*)(sBestD + cap);                                          // [cap]
    int* sBestI = sLabel + cap;                                                  // [cap]; behind the hull: the vertices' indices
    __shared__ int sWave[MG_THREADS / 64], sN, sFlag, sCnt[2];
    const int tid = threadIdx.x, lane = tid & 63, nC = A.nCams, T = MG_THREADS, N = A.N;
    int pi = 0, pj = 0;
    bool eval = false;   // (uniform in the workgroup)
    if (nC > 1) {
        const int q = blockIdx.x % (nC - 1);
        pi = blockIdx.x / (nC - 1), pj = q + (q >= pi);   // the ordered pair (pi, pj), pi != pj
        if (A.allPairs) eval = true;
        else if (A.groups->groupNum > 1) eval = A.groups->groupId[pi] != A.groups->groupId[pj];   // only cameras of two groups (:59-64)
    }
    if (eval) {
        const int mapCount = A.mapCount ? min(max(*A.mapCount, 0), A.nMap) : A.nMap;
        if (tid == 0) sN = 0, sCnt[0] = 0, sCnt[1] = 0;
        __syncthreads();
        // camera pi's features with a non-false map point (:104-111), in slot order; those that project into camera pj's image (:120-130;
        // no depth test: a point behind pj that projects into the image counts, as in the reference) into LDS
        const double *K = A.K[pj], *R = A.R[pj], *t = A.t[pj];
        const double Wd = (double)A.W, Hd = (double)A.H;
        for (int base = 0; base < N; base += T) {
            const int s = base + tid;
            const int m = s < N ? mg_point(A, pi, s, mapCount) : -1;
            bool in = false;
            double x = 0.0, y = 0.0;
            if (m >= 0) {
                const double M[3] = {A.mapPts[3 * (size_t)m], A.mapPts[3 * (size_t)m + 1], A.mapPts[3 * (size_t)m + 2]};
                const PuProj q = pu_project(K, R, t, M);
                x = q.u / q.w, y = q.v / q.w;                       // project (:124)
                in = x >= 0 && x < Wd && y >= 0 && y < Hd;          // :125
            }
            const unsigned long long bf = __builtin_amdgcn_ballot_w64(m >= 0);
            if (lane == 0 && bf) atomicAdd(&sCnt[0], __popcll(bf));
            const int off = mg_place(in, sWave, &sN);
            if (in && off < cap) sXY[2 * off] = x, sXY[2 * off + 1] = y;
        }
        __syncthreads();
        const int n = sN < cap ? sN : cap, nFeatI = sCnt[0];   // nInCam (at most N <= cap)
        __syncthreads();
        int inNum = -1;
        if (n >= A.minInNum) {   // :136
            int nVert = 0;
            if (n >= 3) {
                hull_quick<MG_THREADS>(sXY, sBestD, sLabel, sBestI, n);   // get2DConvexHull (:139)
                if (tid == 0) sN = 0;
                __syncthreads();
                for (int base = 0; base < n; base += T) {   // the vertices' indices, ascending, into sBestI (off <= k: no slot is read after its write)
                    const int k = base + tid;
                    const bool v = k < n && sLabel[k] <= -2;
                    const int off = mg_place(v, sWave, &sN);
                    if (v) sBestI[off] = k;
                }
                __syncthreads();
                nVert = sN;
            }
            // camera pj's features with a non-false map point, one per lane: the pixel ((int) x, (int) y) against the closed polygon (:150-163)
            for (int base = 0; base < N; base += T) {
                const int s = base + tid;
                const int m = s < N ? mg_point(A, pj, s, mapCount) : -1;
                bool inside = false;
                if (m >= 0 && nVert >= 3) {
                    const double px = (double)(int)A.xy[pj][s], py = (double)(int)A.xy[pj][N + s];   // (x[N] then y[N]; (int): toward zero)
                    inside = true;
                    for (int v = 0; v < nVert; ++v) {
                        const int e = sBestI[v], b = -2 - sLabel[e];
                        if (hull_out(px, py, sXY[2 * e], sXY[2 * e + 1], sXY[2 * b], sXY[2 * b + 1]) > 0) {
                            inside = false;
                            break;
                        }
                    }
                }
                const unsigned long long bi = __builtin_amdgcn_ballot_w64(inside);
                if (lane == 0 && bi) atomicAdd(&sCnt[1], __popcll(bi));
            }
            __syncthreads();
            inNum = sCnt[1];
        }
        if (tid == 0) {
            atomicExch(A.scratch + MG_SCR_IN + pi * MG_MAX_CAMS + pj, n + 1);
            atomicExch(A.scratch + MG_SCR_NUM + pi * MG_MAX_CAMS + pj, inNum + 1);
            atomicMax(A.scratch + MG_SCR_FEAT + pi, nFeatI + 1);   // (every workgroup of camera pi has the same count)
        }
    }
    // the workgroup whose ticket is the grid's last: every other workgroup's atomics are behind its own fence
    __threadfence();
    __syncthreads();
    if (tid == 0) sFlag = atomicAdd(A.scratch + MG_SCR_TICKET, 1) == (int)gridDim.x - 1;
    __syncthreads();
    if (!sFlag) return;
    __threadfence();
    if (tid == 0) atomicExch(A.scratch + MG_SCR_TICKET, 0);
    __syncthreads();
    mg_finish(A, sDyn);   // (the points are done with: the tables take their place)
}

}  // namespace

extern "C" size_t cs_merge_check_scratch_bytes(int nCams, int N) {
    (void)nCams, (void)N;   // (the pair tables are sized for 16 cameras; the hull's points live in LDS)
    return MG_SCRATCH_BYTES;
}

extern "C" int cs_merge_check_dev(int device, void* hip_stream, int nCams, const cs_merge_cam* cams, int N, int nMap, const int* d_mapCount,
                                  const double* d_mapPts, const unsigned char* d_mapFlags, int W, int H, const cs_camera_groups* d_groups, int frame,
                                  int minInNum, double minInAreaRatio, double maxCamDist, int allPairs, cs_merge_candidates* d_out, void* d_scratch) {
    const char* who = "cs_merge_check_dev";
    if (nCams < 1 || nCams > MG_MAX_CAMS) {
        cs_set_error("%s: %d cameras (1..%d)", who, nCams, MG_MAX_CAMS);
        return CS_ERR_INVALID;
    }
    if (!cams || N < 1 || nMap < 0 || W < 1 || H < 1 || !d_mapPts || !d_groups || !d_out || !d_scratch) {
        cs_set_error("%s: bad arguments (null table or output, N < 1, nMap < 0)", who);
        return CS_ERR_INVALID;
    }
    MgArgs A;
    memset(&A, 0, sizeof(A));
    A.nCams = nCams, A.N = N, A.nMap = nMap, A.W = W, A.H = H, A.frame = frame, A.minInNum = minInNum, A.allPairs = allPairs ? 1 : 0;
    A.ratio = minInAreaRatio, A.maxCamDist = maxCamDist;
    A.mapCount = d_mapCount, A.mapPts = d_mapPts, A.mapFlags = d_mapFlags, A.groups = d_groups, A.out = d_out, A.scratch = (int*)d_scratch;
    for (int c = 0; c < nCams; ++c) {
        if (!cams[c].xy || !cams[c].state || !cams[c].slot2map || !cams[c].K || !cams[c].R || !cams[c].t) {
            cs_set_error("%s: null pointer in camera %d", who, c);
            return CS_ERR_INVALID;
        }
        A.xy[c] = cams[c].xy, A.state[c] = cams[c].state, A.slot2map[c] = cams[c].slot2map, A.K[c] = cams[c].K, A.R[c] = cams[c].R, A.t[c] = cams[c].t;
    }
    if ((size_t)N * HULL_POINT_BYTES > MG_MAX_LDS) {
        cs_set_error("%s: the hull keeps %d bytes per feature slot in LDS: N = %d does not fit (at most %d)", who, HULL_POINT_BYTES, N,
                     (int)(MG_MAX_LDS / HULL_POINT_BYTES));
        return CS_ERR_INVALID;
    }
    CS_HIP(hipSetDevice(device));
    size_t lds = (size_t)N * HULL_POINT_BYTES;
    lds = lds < MG_FINISH_LDS ? MG_FINISH_LDS : lds;
    if (lds > 64u * 1024u) CS_HIP(hipFuncSetAttribute((const void*)k_merge_check, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    const int blocks = nCams > 1 ? nCams * (nCams - 1) : 1;
    hipLaunchKernelGGL(k_merge_check, dim3(blocks), dim3(MG_THREADS), lds, (hipStream_t)hip_stream, A, N);
    CS_CHECK_LAUNCH();
    return CS_OK;
}

// the synchronous form for a reference-shaped caller (include/shim/app/CoSLAMMergeCheck.h): its own record and scratch on the device for the
// length of the call, the launch, one wait, the record to the host
extern "C" int cs_merge_check(int device, void* hip_stream, int nCams, const cs_merge_cam* cams, int N, int nMap, const int* d_mapCount,
                              const double* d_mapPts, const unsigned char* d_mapFlags, int W, int H, const cs_camera_groups* d_groups, int frame,
                              int minInNum, double minInAreaRatio, double maxCamDist, int allPairs, cs_merge_candidates* h_out) {
    if (!h_out) {
        cs_set_error("cs_merge_check: null output");
        return CS_ERR_INVALID;
    }
    if (nCams < 1 || nCams > MG_MAX_CAMS) {   // (before anything is allocated)
        cs_set_error("cs_merge_check: %d cameras (1..%d)", nCams, MG_MAX_CAMS);
        return CS_ERR_INVALID;
    }
    if (!cams || N < 1 || nMap < 0 || W < 1 || H < 1 || !d_mapPts || !d_groups) {
        cs_set_error("cs_merge_check: bad arguments (null table or output, N < 1, nMap < 0)");
        return CS_ERR_INVALID;
    }
    CS_HIP(hipSetDevice(device));
    char* d = nullptr;
    CS_HIP(hipMalloc((void**)&d, sizeof(cs_merge_candidates) + MG_SCRATCH_BYTES));
    hipStream_t s = (hipStream_t)hip_stream;
    int rc = CS_OK;
    hipError_t e = hipMemsetAsync(d, 0, sizeof(cs_merge_candidates) + MG_SCRATCH_BYTES, s);
    if (e == hipSuccess)
        rc = cs_merge_check_dev(device, hip_stream, nCams, cams, N, nMap, d_mapCount, d_mapPts, d_mapFlags, W, H, d_groups, frame, minInNum,
                                minInAreaRatio, maxCamDist, allPairs, (cs_merge_candidates*)d, d + sizeof(cs_merge_candidates));
    if (e == hipSuccess && rc == CS_OK) e = hipMemcpyAsync(h_out, d, sizeof(cs_merge_candidates), hipMemcpyDeviceToHost, s);
    if (e == hipSuccess && rc == CS_OK) e = hipStreamSynchronize(s);
    (void)hipFree(d);
    if (rc != CS_OK) return rc;
    if (e != hipSuccess) {
        cs_set_error("cs_merge_check: %s", hipGetErrorString(e));
        return CS_ERR_HIP;
    }
    return CS_OK;
}
