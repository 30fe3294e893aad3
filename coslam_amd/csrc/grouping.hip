// grouping.hip -- CoSLAM::cameraGrouping with CoSLAM::getViewOverlapCosts under it, per frame, on the device (gfx950).
//
// Replaces getViewOverlapCosts (src/app/SL_CoSLAM.cpp:1543-1630) and cameraGrouping (:1632-1697).  The reference walks curMapPts on the
// host, pushes every shared feature's pixel into sharedPoints[i][j], takes the convex hull and polygon area of each of the nCams^2 sets
// (get2DConvexHull / getPolyArea: LibVisualSLAM functions that are not in the reference tree -- here the convex hull and its shoelace
// area) and walks the cost graph's connected components with an explicit stack.
//
// Two paths:
//   counting   k_group_count: a grid over the rows of the hand-back's pointFeat table (the listed ones, or all rows below the map count).
//              A lane forms the bit mask of the cameras that hold its point in this frame; 16 ballots per 64 rows give every camera's lane
//              set, a pair's count is the popcount of two of them, kept in registers over the whole grid-stride loop; a 1 KB LDS table of
//              integers per workgroup, integer vector atomics to the global table.  Integers only: the result does not depend on the order
//              of arrival.  minOverlapAreaRatio <= 0 can never cut a pair (an area is never < 0), so the per-frame call stops here.
//   hull       k_group_hull: one workgroup per ORDERED camera pair compacts camera i's pixels of the shared points into LDS in row order and
//              runs Quickhull rounds over them in parallel (hull_quick, hull_dev.h: shared with merge.hip): every point outside the current polygon belongs to one edge, every edge takes
//              its farthest point (LDS 64-bit max of the f64 distance's bits, lowest index among equals) and splits, points inside the
//              new polygon drop out.  An edge is named by its start vertex and keeps its data in that point's slot, so the whole state is
//              32 bytes per point.  Each split adds the triangle (a, f, b) to the polygon: the area is half the sum of the winners' cross
//              products, summed per thread in round order and then up a fixed tree -- the same on every call.
// The thresholds, the distance cut and the component walk are a few hundred scalar operations: the workgroup whose ticket (an integer
// vector atomic on global memory) comes last does them.  It also leaves the scratch counters zero for the next call.
#include "cs_common.h"
#include "hull_dev.h"

namespace {

constexpr int GR_MAX_CAMS = 16;
constexpr int GR_TAB = GR_MAX_CAMS * GR_MAX_CAMS;
constexpr int GR_COUNT_THREADS = 256;
constexpr int GR_HULL_THREADS = 1024;
constexpr int GR_HULL_POINT_BYTES = HULL_POINT_BYTES;   // (hull_dev.h)
constexpr size_t GR_MAX_LDS = 160u * 1024u - 1024u;   // a workgroup's LDS on gfx950, less the hull kernel's static words
constexpr int GR_REC = 336;                       // ints: gr_finish's neighbour masks, stack and cs_camera_groups record
constexpr size_t GR_FINISH_LDS = GR_TAB * (sizeof(int) + sizeof(double)) + GR_REC * sizeof(int);   // gr_finish's tables
// scratch (ints): [0, 256) pair counters, [256] ticket; then (8-byte aligned) 256 doubles of hull areas
constexpr int GR_SCR_TICKET = GR_TAB;
constexpr int GR_SCR_AREA_OFF = (GR_TAB + 2) * (int)sizeof(int);
constexpr size_t GR_SCRATCH_BYTES = GR_SCR_AREA_OFF + GR_TAB * sizeof(double);

struct GrArgs {
    int nCams, N, nMap, W, H, minNum, hull, finishHere;
    double ratio, maxDist;        // maxDist = m_initCamTranslation * Param::maxDistRatio
    const int* mapCount;
    const int* pointFeat;
    const unsigned char* mapFlags;
    const int* list;
    const int* listCount;
    double* vcosts;
    int* nShare;
    double* hullArea;
    cs_camera_groups* groups;     // null: getViewOverlapCosts only
    int* scratch;
    const double* xy[GR_MAX_CAMS];
    const double* R[GR_MAX_CAMS];
    const double* t[GR_MAX_CAMS];
};

__device__ __forceinline__ int gr_rows(const GrArgs& A) {
    int n = A.mapCount ? *A.mapCount : A.nMap;
    n = n < 0 ? 0 : (n > A.nMap ? A.nMap : n);
    if (!A.list) return n;
    int m = A.listCount ? *A.listCount : A.nMap;
    return m < 0 ? 0 : (m > A.nMap ? A.nMap : m);
}
// the k-th row to look at, or -1: below the map count, not false (SL_CoSLAM.cpp:1563)
__device__ __forceinline__ int gr_row(const GrArgs& A, int k, int mapCount) {
    int r = k;
    if (A.list) r = A.list[k];
    if (r < 0 || r >= mapCount) return -1;
    if (A.mapFlags && (A.mapFlags[r] & CS_MAP_FALSE)) return -1;
    return r;
}

// vcosts (:1606-1629), the distance cut (:1638-1655), the components (:1659-1695): one workgroup, after every count and area has landed
__device__ void gr_finish(const GrArgs& A, int* sTab, double* sCost, int* sRec) {
    const int tid = threadIdx.x, nC = A.nCams;
    const double* area = (const double*)((const char*)A.scratch + GR_SCR_AREA_OFF);
    // the pair's distance test (:1638-1655; getCamCenter: -R^T t) first: its loads travel with the counters' exchange below
    bool far = false;
    if (A.groups && tid < nC * nC && tid / nC < tid % nC) {
        const int i = tid / nC, j = tid % nC;
        double Ci[3], Cj[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            Ci[k] = -((A.R[i][k] * A.t[i][0] + A.R[i][3 + k] * A.t[i][1]) + A.R[i][6 + k] * A.t[i][2]);
            Cj[k] = -((A.R[j][k] * A.t[j][0] + A.R[j][3 + k] * A.t[j][1]) + A.R[j][6 + k] * A.t[j][2]);
        }
        const double dx = Ci[0] - Cj[0], dy = Ci[1] - Cj[1], dz = Ci[2] - Cj[2];
        far = sqrt((dx * dx + dy * dy) + dz * dz) > A.maxDist;
    }
    for (int e = tid; e < GR_TAB; e += blockDim.x) sTab[e] = atomicExch(A.scratch + e, 0);   // (the value in L2, and zero for the next call)
    __syncthreads();
    for (int e = tid; e < nC * nC; e += blockDim.x) {
        const int i = e / nC, j = e % nC;
        const int n = i == j ? 0 : sTab[i * GR_MAX_CAMS + j];
        double c = -1.0, aij = 0.0;
        if (i != j) {
            if (A.hull) {
                aij = __hip_atomic_load(area + i * GR_MAX_CAMS + j, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                const double aji = __hip_atomic_load(area + j * GR_MAX_CAMS + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                const double a1 = i < j ? aij : aji, a2 = i < j ? aji : aij;   // area1 = hull(lower, higher), :1615-1616
                const double full = (double)A.W * (double)A.H;
                if (!(n < A.minNum) && !(a1 < A.ratio * full || a2 < A.ratio * full)) c = (double)n;   // :1609, :1621
            } else if (!(n < A.minNum))
                c = (double)n;
        }
        sCost[e] = c;
        A.nShare[e] = n;
        if (A.hullArea) A.hullArea[e] = aij;
    }
    __syncthreads();
    if (far && sCost[tid] > 0) {   // a positive cost between cameras too far apart is cut (nC * nC <= 256 <= blockDim.x; only i < j threads)
        const int i = tid / nC, j = tid % nC;
        sCost[i * nC + j] = -1.0, sCost[j * nC + i] = -1.0;
    }
    __syncthreads();
    for (int e = tid; e < nC * nC; e += blockDim.x) A.vcosts[e] = sCost[e];
    if (!A.groups) return;
    // :1659-1695, the explicit stack as written: the order inside a group is the order of discovery.  One lane walks; it reads a camera's
    // neighbours as a bit mask (one LDS word per popped camera) and builds the record in LDS, which the workgroup then stores
    int *sAdj = sRec, *sVQ = sRec + GR_MAX_CAMS, *sG = sRec + 2 * GR_MAX_CAMS;   // neighbour masks, the stack, the cs_camera_groups record as ints
    constexpr int G_WORDS = (int)(sizeof(cs_camera_groups) / sizeof(int));
    static_assert(G_WORDS + 2 * GR_MAX_CAMS <= GR_REC, "gr_finish's record buffer");
    constexpr int G_NUM = 1, G_IDS = 1 + GR_MAX_CAMS, G_GID = G_IDS + GR_MAX_CAMS * GR_MAX_CAMS;
    int adj = 0;
    if (tid < nC)
        for (int j = 0; j < nC; ++j) adj |= (j != tid && sCost[tid * nC + j] > 0) << j;
    if (tid < nC) sAdj[tid] = adj;
    for (int e = tid; e < G_WORDS; e += blockDim.x) sG[e] = e >= G_NUM && e < G_IDS ? 0 : -1;
    __syncthreads();
    if (tid == 0) {
        int nVQ, flag = 0, g = 0;
        for (int i = 0; i < nC; ++i) {
            if (flag >> i & 1) continue;       // :1665
            int nCON = 0;
            nVQ = 0;
            sG[G_IDS + g * GR_MAX_CAMS + nCON++] = i, sG[G_GID + i] = g, sVQ[nVQ++] = i, flag |= 1 << i;   // :1667-1670
            while (nVQ > 0) {
                const int iCam = sVQ[--nVQ];    // :1674-1675
                int cand = sAdj[iCam] & ~flag; // :1678-1680, j ascending
                flag |= cand;
                while (cand) {
                    const int j = __ffs(cand) - 1;
                    cand &= cand - 1;
                    sG[G_IDS + g * GR_MAX_CAMS + nCON++] = j, sG[G_GID + j] = g, sVQ[nVQ++] = j;   // :1681-1683
                }
            }
            sG[G_NUM + g++] = nCON;
        }
        sG[0] = g;
    }
    __syncthreads();
    int* out = (int*)A.groups;
    for (int e = tid; e < G_WORDS; e += blockDim.x) out[e] = sG[e];
}

// the workgroup whose ticket is the grid's last: every other workgroup's atomics and stores are behind its own fence
__device__ __forceinline__ bool gr_last(const GrArgs& A, int* sFlag) {
    __threadfence();
    __syncthreads();
    if (threadIdx.x == 0) *sFlag = atomicAdd(A.scratch + GR_SCR_TICKET, 1) == (int)gridDim.x - 1;
    __syncthreads();
    if (!*sFlag) return false;
    __threadfence();
    if (threadIdx.x == 0) atomicExch(A.scratch + GR_SCR_TICKET, 0);
    return true;
}

__global__ __launch_bounds__(GR_COUNT_THREADS) void k_group_count(GrArgs A) {
    __shared__ int sTab[GR_TAB], sRec[GR_REC], sFlag;
    __shared__ double sCost[GR_TAB];
    const int tid = threadIdx.x, lane = tid & 63, nC = A.nCams;
    sTab[tid] = 0;
    __syncthreads();
    // the counts on the device are read here and looked at BEHIND the rows' loads: the loop runs to the host's bound, so that the table's rows
    // are on their way while the counts arrive (one dependent global round less on a launch that is a chain of a few such rounds)
    const int mapCountRaw = A.mapCount ? *A.mapCount : A.nMap, listCountRaw = A.list && A.listCount ? *A.listCount : A.nMap;
    // lane L keeps the counts of table entries L, L + 64, L + 128, L + 192 (entry = i * 16 + j)
    int acc0 = 0, acc1 = 0, acc2 = 0, acc3 = 0;
    const int j0 = lane & 15, i0 = lane >> 4;
    for (int base = blockIdx.x * GR_COUNT_THREADS; base < A.nMap; base += gridDim.x * GR_COUNT_THREADS) {   // (uniform per workgroup)
        const int k = base + tid;
        int r = -1;
        if (k < A.nMap) {
            r = A.list ? A.list[k] : k;
            if (r >= A.nMap) r = -1;
        }
        unsigned mask = 0;
        if (r >= 0) {
            const int* pf = A.pointFeat + (size_t)r * nC;
            for (int c = 0; c < nC; ++c) mask |= (unsigned)(pf[c] >= 0) << c;   // a feature of THIS frame (:1570)
            if (A.mapFlags && (A.mapFlags[r] & CS_MAP_FALSE)) mask = 0;         // isFalse() (:1563)
        }
        if (k >= listCountRaw || r >= mapCountRaw) mask = 0;                    // behind the list / not a map point
        unsigned long long mine = 0;   // lane c: the lanes whose point camera c holds
        for (int c = 0; c < nC; ++c) {
            const unsigned long long b = __builtin_amdgcn_ballot_w64(mask >> c & 1);
            if (lane == c) mine = b;
        }
        const unsigned long long bj = __shfl(mine, j0, 64);
        acc0 += __popcll(__shfl(mine, i0, 64) & bj);
        acc1 += __popcll(__shfl(mine, i0 + 4, 64) & bj);
        acc2 += __popcll(__shfl(mine, i0 + 8, 64) & bj);
        acc3 += __popcll(__shfl(mine, i0 + 12, 64) & bj);
    }
    if (acc0 && i0 != j0) atomicAdd(&sTab[lane], acc0);
    if (acc1 && i0 + 4 != j0) atomicAdd(&sTab[lane + 64], acc1);
    if (acc2 && i0 + 8 != j0) atomicAdd(&sTab[lane + 128], acc2);
    if (acc3 && i0 + 12 != j0) atomicAdd(&sTab[lane + 192], acc3);
    __syncthreads();
    if (sTab[tid]) atomicAdd(A.scratch + tid, sTab[tid]);
    if (!A.finishHere) return;
    if (!gr_last(A, &sFlag)) return;
    gr_finish(A, sTab, sCost, sRec);
}

// one wave, nothing to count: a rig of one camera (the reference returns early, :1633)
__global__ __launch_bounds__(GR_COUNT_THREADS) void k_group_finish(GrArgs A) {
    __shared__ int sTab[GR_TAB], sRec[GR_REC];
    __shared__ double sCost[GR_TAB];
    gr_finish(A, sTab, sCost, sRec);
}

__global__ __launch_bounds__(GR_HULL_THREADS) void k_group_hull(GrArgs A, int cap) {
    extern __shared__ double sDyn[];
    // per point: xy, the label (alive: its edge = that edge's start vertex >= 0; dead: -1; a vertex: -2 - next vertex), and in a vertex's
    // slot its edge's best distance and best index of the round
    double* sXY = sDyn;                                          // [cap][2]
    unsigned long long* sBestD = (unsigned long long*)(sXY + 2 * (size_t)cap);   // [cap]
    int* sLabel = (int*)(sBestD + cap);                          // [cap]
    int* sBestI = sLabel + cap;                                  // [cap]
    __shared__ int sWave[GR_HULL_THREADS / 64], sN, sFlag;
    __shared__ double sRed[GR_HULL_THREADS / 64];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, nC = A.nCams, T = GR_HULL_THREADS;
    const int pi = blockIdx.x / (nC - 1), q = blockIdx.x % (nC - 1), pj = q + (q >= pi);   // the ordered pair (pi, pj), pi != pj
    const int mapCount = A.mapCount ? min(max(*A.mapCount, 0), A.nMap) : A.nMap, rows = gr_rows(A);
    if (tid == 0) sN = 0;
    __syncthreads();
    // camera pi's pixels of the points both cameras hold, in row order; counted past cap, never written past it
    for (int base = 0; base < rows; base += T) {
        const int k = base + tid;
        const int r = k < rows ? gr_row(A, k, mapCount) : -1;
        int s = -1;
        if (r >= 0) {
            const int si = A.pointFeat[(size_t)r * nC + pi], sj = A.pointFeat[(size_t)r * nC + pj];
            if (si >= 0 && sj >= 0 && si < A.N) s = si;
        }
        const unsigned long long b = __builtin_amdgcn_ballot_w64(s >= 0);
        if (lane == 0) sWave[wv] = __popcll(b);
        __syncthreads();
        int off = sN;
        for (int w = 0; w < wv; ++w) off += sWave[w];
        off += __popcll(b & ((1ull << lane) - 1ull));
        if (s >= 0 && off < cap) sXY[2 * off] = A.xy[pi][s], sXY[2 * off + 1] = A.xy[pi][A.N + s];   // (x[N] then y[N])
        __syncthreads();
        if (tid == 0) {
            int tot = sN;
            for (int w = 0; w < T / 64; ++w) tot += sWave[w];
            sN = tot;
        }
        __syncthreads();
    }
    const int nAll = sN, n = nAll < cap ? nAll : cap;
    double acc = 0.0;
    if (nAll <= cap && n >= 3) acc = hull_quick<GR_HULL_THREADS>(sXY, sBestD, sLabel, sBestI, n);   // (the rounds: hull_dev.h)
    // the threads' sums up a fixed tree
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
    if (lane == 0) sRed[wv] = acc;
    __syncthreads();
    if (tid == 0) {
        double s = 0.0;
        for (int w = 0; w < T / 64; ++w) s += sRed[w];
        double* area = (double*)((char*)A.scratch + GR_SCR_AREA_OFF);
        // more shared points than slots: no hull over a truncated set -- the pair's area reads -1 (below every positive threshold)
        __hip_atomic_store(area + pi * GR_MAX_CAMS + pj, nAll > cap ? -1.0 : 0.5 * s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    if (!gr_last(A, &sFlag)) return;
    gr_finish(A, (int*)(sDyn + GR_TAB), sDyn, (int*)(sDyn + GR_TAB) + GR_TAB);   // (the points are done with: the tables take their place)
}

int gr_fill(GrArgs& A, const char* who, int nCams, const cs_grouping_cam* cams, int N, int nMap, const int* d_mapCount, const int* d_pointFeat,
            const unsigned char* d_mapFlags, const int* d_list, const int* d_listCount, int W, int H, int minOverlapNum, double minOverlapAreaRatio,
            double* d_vcosts, int* d_nShare, double* d_hullArea, void* d_scratch) {
    if (nCams < 1 || nCams > GR_MAX_CAMS) {
        cs_set_error("%s: %d cameras (1..%d)", who, nCams, GR_MAX_CAMS);
        return CS_ERR_INVALID;
    }
    if (!cams || N < 1 || nMap < 0 || W < 1 || H < 1 || !d_pointFeat || !d_vcosts || !d_nShare || !d_scratch) {
        cs_set_error("%s: bad arguments (null table or output, N < 1, nMap < 0)", who);
        return CS_ERR_INVALID;
    }
    memset(&A, 0, sizeof(A));
    A.nCams = nCams, A.N = N, A.nMap = nMap, A.W = W, A.H = H, A.minNum = minOverlapNum, A.ratio = minOverlapAreaRatio;
    A.hull = (minOverlapAreaRatio > 0 || d_hullArea) ? 1 : 0;
    A.mapCount = d_mapCount, A.pointFeat = d_pointFeat, A.mapFlags = d_mapFlags, A.list = d_list, A.listCount = d_listCount;
    A.vcosts = d_vcosts, A.nShare = d_nShare, A.hullArea = d_hullArea, A.scratch = (int*)d_scratch;
    for (int c = 0; c < nCams; ++c) {
        if (!cams[c].xy || !cams[c].R || !cams[c].t) {
            cs_set_error("%s: null pointer in camera %d", who, c);
            return CS_ERR_INVALID;
        }
        A.xy[c] = cams[c].xy, A.R[c] = cams[c].R, A.t[c] = cams[c].t;
    }
    if (A.hull && nCams > 1 && (size_t)N * GR_HULL_POINT_BYTES > GR_MAX_LDS) {
        cs_set_error("%s: the hull path keeps %d bytes per feature slot in LDS: N = %d does not fit (at most %d)", who, GR_HULL_POINT_BYTES, N,
                     (int)(GR_MAX_LDS / GR_HULL_POINT_BYTES));
        return CS_ERR_INVALID;
    }
    return CS_OK;
}

int gr_launch(GrArgs& A, int device, void* hip_stream) {
    CS_HIP(hipSetDevice(device));
    hipStream_t s = (hipStream_t)hip_stream;
    if (A.nCams == 1) {
        hipLaunchKernelGGL(k_group_finish, dim3(1), dim3(GR_COUNT_THREADS), 0, s, A);
        CS_CHECK_LAUNCH();
        return CS_OK;
    }
    int blocks = (A.nMap + GR_COUNT_THREADS - 1) / GR_COUNT_THREADS;
    blocks = blocks < 1 ? 1 : (blocks > 128 ? 128 : blocks);
    A.finishHere = A.hull ? 0 : 1;
    hipLaunchKernelGGL(k_group_count, dim3(blocks), dim3(GR_COUNT_THREADS), 0, s, A);
    if (A.hull) {
        size_t lds = (size_t)A.N * GR_HULL_POINT_BYTES;
        lds = lds < GR_FINISH_LDS ? GR_FINISH_LDS : lds;
        if (lds > 64u * 1024u) CS_HIP(hipFuncSetAttribute((const void*)k_group_hull, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        hipLaunchKernelGGL(k_group_hull, dim3(A.nCams * (A.nCams - 1)), dim3(GR_HULL_THREADS), lds, s, A, A.N);
    }
    CS_CHECK_LAUNCH();
    return CS_OK;
}

}  // namespace

extern "C" size_t cs_camera_grouping_scratch_bytes(int nCams, int N) {
    (void)nCams, (void)N;   // (the pair tables are sized for 16 cameras; the hull's points live in LDS)
    return GR_SCRATCH_BYTES;
}

extern "C" int cs_view_overlap_costs_dev(int device, void* hip_stream, int nCams, const cs_grouping_cam* cams, int N, int nMap, const int* d_mapCount,
                                         const int* d_pointFeat, const unsigned char* d_mapFlags, const int* d_list, const int* d_listCount, int W,
                                         int H, int minOverlapNum, double minOverlapAreaRatio, double* d_vcosts, int* d_nShare, double* d_hullArea,
                                         void* d_scratch) {
    GrArgs A;
    const int rc = gr_fill(A, "cs_view_overlap_costs_dev", nCams, cams, N, nMap, d_mapCount, d_pointFeat, d_mapFlags, d_list, d_listCount, W, H,
                           minOverlapNum, minOverlapAreaRatio, d_vcosts, d_nShare, d_hullArea, d_scratch);
    if (rc != CS_OK) return rc;
    return gr_launch(A, device, hip_stream);
}

extern "C" int cs_camera_grouping_dev(int device, void* hip_stream, int nCams, const cs_grouping_cam* cams, int N, int nMap, const int* d_mapCount,
                                      const int* d_pointFeat, const unsigned char* d_mapFlags, const int* d_list, const int* d_listCount, int W, int H,
                                      int minOverlapNum, double minOverlapAreaRatio, double* d_vcosts, int* d_nShare, double* d_hullArea,
                                      void* d_scratch, double initCamTranslation, double maxDistRatio, cs_camera_groups* d_groups) {
    GrArgs A;
    const int rc = gr_fill(A, "cs_camera_grouping_dev", nCams, cams, N, nMap, d_mapCount, d_pointFeat, d_mapFlags, d_list, d_listCount, W, H,
                           minOverlapNum, minOverlapAreaRatio, d_vcosts, d_nShare, d_hullArea, d_scratch);
    if (rc != CS_OK) return rc;
    if (!d_groups) {
        cs_set_error("cs_camera_grouping_dev: d_groups is null");
        return CS_ERR_INVALID;
    }
    A.groups = d_groups, A.maxDist = initCamTranslation * maxDistRatio;
    return gr_launch(A, device, hip_stream);
}
