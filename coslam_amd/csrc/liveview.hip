// liveview.hip -- the frame's last step on the device (gfx950): CoSLAM::getNumDynamicStaticPoints, CoSLAM::storeDynamicPoints and the
// display's getDynTracks, with a snapshot of the frame streamed to the host.
//
// Replaces getNumDynamicStaticPoints (src/app/SL_CoSLAM.cpp:1447-1471), storeDynamicPoints (:1900-1911) and getDynTracks
// (src/gui/GLScenePane.cpp:19-52).  The reference walks curMapPts on the host three times per frame (the counts, the dynamic list, the
// display's copy) and getDynTracks rebuilds a std::map over the whole of m_dynPts for every redraw.  DESIGN 3.18.
//
//   k_live_frame   one launch per frame.  A workgroup owns a contiguous stretch of the map's rows, so the order of the lists is the order of
//                  the workgroups: it counts with ballots (integers: 34 LDS counters per workgroup, integer vector atomics to the global
//                  ones), compacts its rows that take part / are dynamic IN ORDER into its own stretch of two staging tables and leaves its
//                  two run lengths.  Nobody waits for anybody: the workgroup whose ticket (an integer vector atomic on global memory) comes
//                  last sums the run lengths, and places the runs: the dynamic list into the frame's slot of the device ring, and -- on a
//                  publishing frame -- the header and the records into the pinned host slot, with plain stores (as k_hostview_pack).  The
//                  caps cut the lists while they are placed; nothing is staged or placed on behalf of a list nobody asked for (the
//                  current list on a frame that is not published, the dynamic list of a one-camera rig, both in the counts-only mode).
//   k_live_trails  one wave per trail, one lane per (trail, frame): the lists are ascending in id by construction, so a lane finds its id in
//                  its frame's list by binary search; a ballot's prefix count is the position inside the trail, which skips the gaps.
// Figures of the compiler (hipcc -O3, gfx950): k_live_frame 44 VGPRs, 2348 bytes of LDS, no scratch; k_live_trails 16 VGPRs, no LDS, no scratch.
#include <vector>

#include "cs_common.h"

namespace {

constexpr int LV_MAX_CAMS = 16;
constexpr int LV_THREADS = 256;
constexpr int LV_MAX_BLOCKS = 256;         // (<= LV_THREADS: a thread of the last workgroup per workgroup)
constexpr int LV_ROWS = 1024;              // rows of a workgroup, at least
constexpr int LV_NCNT = 2 * LV_MAX_CAMS + 2;   // [0, 16) static features per camera, [16, 32) dynamic ones, [32] nStatic, [33] nDynamic
// scratch (ints): [0, 34) the counters, [34] the ticket, [64, 320) the workgroups' current runs, [320, 576) their dynamic runs
constexpr int LV_SCR_TICKET = LV_NCNT;
constexpr int LV_SCR_CUR = 64;
constexpr int LV_SCR_DYN = LV_SCR_CUR + LV_MAX_BLOCKS;
constexpr int LV_SCR_INTS = LV_SCR_DYN + LV_MAX_BLOCKS;
constexpr int LV_STAGE_ROWS = 65536;       // staging rows of a new view

static_assert(sizeof(cs_live_point) == 32 && sizeof(cs_live_dyn) == 32, "record sizes");
static_assert(sizeof(cs_live_header) % 8 == 0 && sizeof(cs_map_counts) == LV_NCNT * sizeof(int), "header layout");

struct LvArgs {
    int nCams, nMap, rowsPerBlock, frame, every;
    int lists;       // 0: counts only
    int publish;     // the current list and the header go to the host slot
    int curCap, dynCap;
    const int* mapCount;
    const int* pointFeat;
    const unsigned char* mapFlags;
    const double* mapPts;
    const double* R;
    const double* t;
    const cs_camera_groups* groups;
    int* scratch;
    int2* stageCur;          // [nMap] {row, camMask | flags << 16 | numVisCam << 24}
    int* stageDyn;           // [nMap] row
    cs_live_dyn* dynOut;     // this frame's slot of the device ring
    int* dynCount;
    int* dynFrame;
    cs_live_header* hdr;     // this frame's slot of the pinned ring (device pointers), publishing frames only
    cs_live_point* pts;
    cs_map_counts* counts;   // counts-only mode
    int* totals;             // [2] the view's running overflow totals: current (published frames), dynamic (all frames)
};

// the workgroup whose ticket is the grid's last: every other workgroup's atomics and stores are behind its own fence
__device__ __forceinline__ bool lv_last(const LvArgs& A, int* sFlag) {
    __threadfence();
    __syncthreads();
    if (threadIdx.x == 0) *sFlag = atomicAdd(A.scratch + LV_SCR_TICKET, 1) == (int)gridDim.x - 1;
    __syncthreads();
    if (!*sFlag) return false;
    __threadfence();
    if (threadIdx.x == 0) atomicExch(A.scratch + LV_SCR_TICKET, 0);
    return true;
}

// the workgroup that holds entry e of a list: the last one whose run starts at or before e (runs of length 0 start where the next one does)
__device__ __forceinline__ int lv_find(const int* off, int nb, int e) {
    int lo = 0, hi = nb - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (off[mid] <= e) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

__global__ __launch_bounds__(LV_THREADS) void k_live_frame(LvArgs A) {
    __shared__ int sCnt[64], sWave[2][LV_THREADS / 64], sFlag, sOffC[LV_MAX_BLOCKS], sOffD[LV_MAX_BLOCKS], sTot[2];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, nC = A.nCams;
    if (tid < 64) sCnt[tid] = 0;
    __syncthreads();
    // the count on the device is looked at BEHIND the rows' loads (as k_group_count): the loop runs to the host's bound
    const int mapCountRaw = A.mapCount ? *A.mapCount : A.nMap;
    const int mapCount = mapCountRaw < 0 ? 0 : (mapCountRaw > A.nMap ? A.nMap : mapCountRaw);
    const int r0 = blockIdx.x * A.rowsPerBlock, r1 = min(r0 + A.rowsPerBlock, A.nMap);
    const bool wantCur = A.lists && A.publish, wantDyn = A.lists && nC > 1;   // one camera: no dynamic list (:1901-1902)
    const unsigned long long below = (1ull << lane) - 1ull;
    int acc = 0, runC = 0, runD = 0;
    for (int base = r0; base < r1; base += LV_THREADS) {   // (uniform per workgroup)
        const int r = base + tid;
        unsigned mask = 0, fl = 0;
        if (r < r1) {
            const int* pf = A.pointFeat + (size_t)r * nC;
            for (int c = 0; c < nC; ++c) mask |= (unsigned)(pf[c] >= 0) << c;   // a feature of THIS frame: pFeatures[c] (:1463)
            if (A.mapFlags) fl = A.mapFlags[r];
        }
        if (r >= mapCount) mask = 0;   // not a map point
        const bool part = mask != 0;                                   // on curMapPts
        const bool isS = part && fl == 0, isD = part && fl == CS_MAP_DYNAMIC;   // isCertainStatic / isCertainDynamic
        for (int c = 0; c < nC; ++c) {
            const unsigned long long bS = __builtin_amdgcn_ballot_w64(isS && (mask >> c & 1));
            const unsigned long long bD = __builtin_amdgcn_ballot_w64(isD && (mask >> c & 1));
            if (lane == c) acc += __popcll(bS);
            if (lane == LV_MAX_CAMS + c) acc += __popcll(bD);
        }
        const unsigned long long bs = __builtin_amdgcn_ballot_w64(isS), bd = __builtin_amdgcn_ballot_w64(isD);
        if (lane == 2 * LV_MAX_CAMS) acc += __popcll(bs);
        if (lane == 2 * LV_MAX_CAMS + 1) acc += __popcll(bd);
        if (!A.lists) continue;
        // the rows that take part and the dynamic ones, each in row order, into this workgroup's stretch of the staging tables
        const unsigned long long bc = __builtin_amdgcn_ballot_w64(part);
        if (lane == 0) sWave[0][wv] = __popcll(bc), sWave[1][wv] = __popcll(bd);
        __syncthreads();
        int oc = runC, od = runD;
#pragma unroll
        for (int w = 0; w < LV_THREADS / 64; ++w) {
            if (w < wv) oc += sWave[0][w], od += sWave[1][w];
            runC += sWave[0][w], runD += sWave[1][w];
        }
        if (wantCur && part) A.stageCur[r0 + oc + __popcll(bc & below)] = make_int2(r, (int)(mask | fl << 16 | (unsigned)__popc(mask) << 24));
        if (wantDyn && isD) A.stageDyn[r0 + od + __popcll(bd & below)] = r;
        __syncthreads();   // (sWave is rewritten by the next round)
    }
    if (acc && lane < LV_NCNT) atomicAdd(&sCnt[lane], acc);
    __syncthreads();
    if (tid < LV_NCNT && sCnt[tid]) atomicAdd(A.scratch + tid, sCnt[tid]);
    if (A.lists && tid == 0) {
        __hip_atomic_store(A.scratch + LV_SCR_CUR + blockIdx.x, runC, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(A.scratch + LV_SCR_DYN + blockIdx.x, runD, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    if (!lv_last(A, &sFlag)) return;

    // ---- the last workgroup: the totals (the value in L2, and zero for the next call), the runs' places, the lists
    const int nb = gridDim.x;
    if (tid < 64) sCnt[tid] = tid < LV_NCNT ? atomicExch(A.scratch + tid, 0) : 0;
    if (A.lists && tid < nb) {
        sOffC[tid] = __hip_atomic_load(A.scratch + LV_SCR_CUR + tid, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        sOffD[tid] = __hip_atomic_load(A.scratch + LV_SCR_DYN + tid, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    __syncthreads();
    // cs_map_counts' order: nStatic, nDynamic, nStaticFeat[16], nDynamicFeat[16]
    const int cntOfWord = tid < 2 ? 2 * LV_MAX_CAMS + tid : tid - 2;
    if (A.counts && tid < LV_NCNT) ((int*)A.counts)[tid] = sCnt[cntOfWord];
    if (!A.lists) return;
    int offC = 0, offD = 0, cntC = 0, cntD = 0;
    if (tid < nb) {
        for (int w = 0; w < tid; ++w) offC += sOffC[w], offD += sOffD[w];
        cntC = sOffC[tid], cntD = sOffD[tid];
    }
    __syncthreads();
    if (tid < nb) {
        sOffC[tid] = offC, sOffD[tid] = offD;
        if (tid == nb - 1) sTot[0] = offC + cntC, sTot[1] = offD + cntD;
    }
    __syncthreads();
    const int totC = sTot[0], totD = wantDyn ? sTot[1] : 0;
    const int keepC = totC < A.curCap ? totC : A.curCap, keepD = totD < A.dynCap ? totD : A.dynCap;
    for (int e = tid; e < keepD; e += LV_THREADS) {   // storeDynamicPoints (:1905-1909)
        const int b = lv_find(sOffD, nb, e);
        const int r = A.stageDyn[b * A.rowsPerBlock + (e - sOffD[b])];
        const double* M = A.mapPts + (size_t)r * 3;
        cs_live_dyn d;
        d.x = M[0], d.y = M[1], d.z = M[2], d.id = r, d.reserved = 0;
        A.dynOut[e] = d;
    }
    if (tid == 0) {   // (one workgroup per frame and the frames one behind the other: plain read-modify-write)
        *A.dynCount = keepD, *A.dynFrame = A.frame;
        A.totals[1] += totD - keepD;
        if (A.publish) A.totals[0] += totC - keepC;
    }
    if (!A.publish) return;
    for (int e = tid; e < keepC; e += LV_THREADS) {
        const int b = lv_find(sOffC, nb, e);
        const int2 s = A.stageCur[b * A.rowsPerBlock + (e - sOffC[b])];
        const double* M = A.mapPts + (size_t)s.x * 3;
        cs_live_point p;
        p.M[0] = M[0], p.M[1] = M[1], p.M[2] = M[2], p.id = s.x;
        p.camMask = (unsigned short)(s.y & 0xffff), p.flags = (unsigned char)(s.y >> 16 & 0xff), p.numVisCam = (unsigned char)(s.y >> 24 & 0xff);
        A.pts[e] = p;
    }
    cs_live_header* h = A.hdr;
    if (tid == 0) {
        h->frame = A.frame, h->mapCount = mapCount, h->nCur = keepC, h->nDyn = keepD, h->curOverflow = totC - keepC, h->dynOverflow = totD - keepD;
        h->nCams = nC, h->every = A.every, h->curOverflowTotal = A.totals[0], h->dynOverflowTotal = A.totals[1], h->reserved = 0;
    }
    if (tid < LV_NCNT) ((int*)&h->counts)[tid] = sCnt[cntOfWord];
    double* hR = &h->R[0][0];
    double* ht = &h->t[0][0];
    for (int e = tid; e < LV_MAX_CAMS * 9; e += LV_THREADS) hR[e] = e < nC * 9 ? A.R[e] : 0.0;
    if (tid < LV_MAX_CAMS * 3) ht[tid] = tid < nC * 3 ? A.t[tid] : 0.0;
    int* hg = (int*)&h->groups;
    const int* g = (const int*)A.groups;
    for (int e = tid; e < (int)(sizeof(cs_camera_groups) / sizeof(int)); e += LV_THREADS) hg[e] = g ? g[e] : 0;
}

struct LtArgs {
    int trjLen, L;           // L = min(trjLen, frames stored): the frames to walk back through, the newest included
    int newest, trailDepth, dynCap;
    const cs_live_dyn* ring;
    const int* count;
    int* nTrails;
    int* trailId;
    int* trailLen;
    double* trailPts;
};

__global__ __launch_bounds__(64) void k_live_trails(LtArgs A) {
    const int lane = threadIdx.x;
    const unsigned long long below = (1ull << lane) - 1ull;
    int n0 = 0;
    if (A.L > 0) {
        n0 = A.count[A.newest];
        n0 = n0 < 0 ? 0 : (n0 > A.dynCap ? A.dynCap : n0);
    }
    if (blockIdx.x == 0 && lane == 0) *A.nTrails = n0;
    for (int i = blockIdx.x; i < n0; i += gridDim.x) {   // the newest frame's ids: ascending, the std::map's order (GLScenePane.cpp:32-36, :48-51)
        const int id = A.ring[(size_t)A.newest * A.dynCap + i].id;
        int run = 0;
        for (int base = 0; base < A.L; base += 64) {
            const int l = base + lane;   // frames back from the newest (:28-30)
            const cs_live_dyn* hit = nullptr;
            if (l < A.L) {
                int slot = (A.newest - l) % A.trailDepth;
                if (slot < 0) slot += A.trailDepth;
                const cs_live_dyn* list = A.ring + (size_t)slot * A.dynCap;
                int n = A.count[slot];
                n = n < 0 ? 0 : (n > A.dynCap ? A.dynCap : n);
                int lo = 0, hi = n;   // the first entry with an id not below ours
                while (lo < hi) {
                    const int mid = (lo + hi) >> 1;
                    if (list[mid].id < id) lo = mid + 1;
                    else hi = mid;
                }
                if (lo < n && list[lo].id == id) hit = list + lo;
            }
            const unsigned long long b = __builtin_amdgcn_ballot_w64(hit != nullptr);
            if (hit) {   // a frame without the id is skipped (:40-43): the position is the count of the frames that hold it
                double* out = A.trailPts + ((size_t)i * A.trjLen + run + __popcll(b & below)) * 3;
                out[0] = hit->x, out[1] = hit->y, out[2] = hit->z;
            }
            run += __popcll(b);
        }
        if (lane == 0) A.trailId[i] = id, A.trailLen[i] = run;
    }
}

void lv_grid(int nMap, int& blocks, int& rowsPerBlock) {
    rowsPerBlock = LV_ROWS;
    if ((long long)nMap > (long long)LV_ROWS * LV_MAX_BLOCKS) {
        rowsPerBlock = (nMap + LV_MAX_BLOCKS - 1) / LV_MAX_BLOCKS;
        rowsPerBlock = (rowsPerBlock + LV_THREADS - 1) / LV_THREADS * LV_THREADS;
    }
    blocks = (nMap + rowsPerBlock - 1) / rowsPerBlock;
    blocks = blocks < 1 ? 1 : blocks;
}

}  // namespace

struct cs_liveview {
    int device, nCams, curCap, dynCap, depth, trailDepth, every;
    int* dScratch;
    int2* dStageCur;
    int* dStageDyn;
    int stageRows;
    cs_live_dyn* dDyn;        // [trailDepth][dynCap]
    int* dDynCount;           // [trailDepth]
    int* dDynFrame;           // [trailDepth]
    int* dTotals;             // [2]
    unsigned char* hRing;     // pinned: depth slots of slotBytes
    unsigned char* dRing;     // the same memory as the device sees it
    size_t slotBytes;
    std::vector<hipEvent_t> landed;
    std::vector<int> frameOf;     // which frame a snapshot slot holds (-1: none)
    long long calls, published;
    int lastFrame;
    // the host form of the trails: device buffers, made at its first call
    int *dTrN, *dTrId, *dTrLen;
    double* dTrPts;
};

static void lv_free(cs_liveview* v) {
    if (!v) return;
    for (void* p : {(void*)v->dScratch, (void*)v->dStageCur, (void*)v->dStageDyn, (void*)v->dDyn, (void*)v->dDynCount, (void*)v->dDynFrame, (void*)v->dTotals,
                    (void*)v->dTrN, (void*)v->dTrId, (void*)v->dTrLen, (void*)v->dTrPts})
        if (p) (void)hipFree(p);
    for (hipEvent_t e : v->landed) (void)hipEventDestroy(e);
    if (v->hRing) (void)hipHostFree(v->hRing);
    delete v;
}

static bool lv_stage(cs_liveview* v, int rows) {
    int2* c = nullptr;
    int* d = nullptr;
    if (hipMalloc((void**)&c, sizeof(int2) * (size_t)rows) != hipSuccess) return false;
    if (hipMalloc((void**)&d, sizeof(int) * (size_t)rows) != hipSuccess) {
        (void)hipFree(c);
        return false;
    }
    if (v->dStageCur) (void)hipFree(v->dStageCur);   // (hipFree waits for the work that uses it)
    if (v->dStageDyn) (void)hipFree(v->dStageDyn);
    v->dStageCur = c, v->dStageDyn = d, v->stageRows = rows;
    return true;
}

extern "C" cs_liveview* cs_liveview_create(int device, int nCams, int curCap, int dynCap, int depth, int trailDepth, int every) {
    if (nCams < 1 || nCams > LV_MAX_CAMS || curCap < 1 || dynCap < 1 || depth < 2 || trailDepth < 1 || every < 1) {
        cs_set_error("cs_liveview_create: bad arguments (1..%d cameras, curCap >= 1, dynCap >= 1, depth >= 2, trailDepth >= 1, every >= 1)",
                     LV_MAX_CAMS);
        return nullptr;
    }
    if (hipSetDevice(device) != hipSuccess) {
        cs_set_error("cs_liveview_create: hipSetDevice(%d) failed", device);
        return nullptr;
    }
    cs_liveview* v = new cs_liveview();
    v->device = device, v->nCams = nCams, v->curCap = curCap, v->dynCap = dynCap, v->depth = depth, v->trailDepth = trailDepth, v->every = every;
    v->dScratch = nullptr, v->dStageCur = nullptr, v->dStageDyn = nullptr, v->stageRows = 0, v->dDyn = nullptr, v->dDynCount = nullptr;
    v->dDynFrame = nullptr, v->dTotals = nullptr, v->hRing = nullptr, v->dRing = nullptr, v->calls = 0, v->published = 0, v->lastFrame = -1;
    v->dTrN = v->dTrId = v->dTrLen = nullptr, v->dTrPts = nullptr;
    v->slotBytes = sizeof(cs_live_header) + sizeof(cs_live_point) * (size_t)curCap;
    const size_t dynBytes = sizeof(cs_live_dyn) * (size_t)trailDepth * dynCap;
    bool ok = hipMalloc((void**)&v->dScratch, sizeof(int) * LV_SCR_INTS) == hipSuccess &&
              hipMemset(v->dScratch, 0, sizeof(int) * LV_SCR_INTS) == hipSuccess && lv_stage(v, LV_STAGE_ROWS) &&
              hipMalloc((void**)&v->dDyn, dynBytes) == hipSuccess && hipMemset(v->dDyn, 0, dynBytes) == hipSuccess &&
              hipMalloc((void**)&v->dDynCount, sizeof(int) * trailDepth) == hipSuccess &&
              hipMemset(v->dDynCount, 0, sizeof(int) * trailDepth) == hipSuccess &&
              hipMalloc((void**)&v->dDynFrame, sizeof(int) * trailDepth) == hipSuccess &&
              hipMemset(v->dDynFrame, 0xff, sizeof(int) * trailDepth) == hipSuccess &&
              hipMalloc((void**)&v->dTotals, sizeof(int) * 2) == hipSuccess && hipMemset(v->dTotals, 0, sizeof(int) * 2) == hipSuccess &&
              hipHostMalloc((void**)&v->hRing, v->slotBytes * depth, hipHostMallocMapped) == hipSuccess;
    if (ok) {
        memset(v->hRing, 0, v->slotBytes * depth);
        ok = hipHostGetDevicePointer((void**)&v->dRing, v->hRing, 0) == hipSuccess;
    }
    v->frameOf.assign(depth, -1);
    for (int s = 0; s < depth && ok; ++s) {
        hipEvent_t e;
        ok = hipEventCreateWithFlags(&e, hipEventDisableTiming) == hipSuccess;
        if (ok) v->landed.push_back(e);
    }
    ok = ok && hipDeviceSynchronize() == hipSuccess;   // (the fills above, before any stream of the caller's uses them)
    if (!ok) {
        cs_set_error("cs_liveview_create: allocation failed (%s)", hipGetErrorString(hipGetLastError()));
        lv_free(v);
        return nullptr;
    }
    return v;
}

extern "C" void cs_liveview_destroy(cs_liveview* v) {
    if (v) (void)hipSetDevice(v->device);
    lv_free(v);
}

extern "C" int cs_liveview_frame_dev(cs_liveview* v, void* hip_stream, int frame, int nMap, const int* d_mapCount, const int* d_pointFeat,
                                     const unsigned char* d_mapFlags, const double* d_mapPts, const double* d_R, const double* d_t,
                                     const cs_camera_groups* d_groups) {
    if (!v || frame < 0 || frame <= v->lastFrame) {
        cs_set_error("cs_liveview_frame_dev: bad arguments (frames must increase: %d after %d)", frame, v ? v->lastFrame : -1);
        return CS_ERR_INVALID;
    }
    if (nMap < 0 || !d_pointFeat || !d_mapPts || !d_R || !d_t) {
        cs_set_error("cs_liveview_frame_dev: bad arguments (null table or poses, nMap < 0)");
        return CS_ERR_INVALID;
    }
    CS_HIP(hipSetDevice(v->device));
    if (nMap > v->stageRows && !lv_stage(v, nMap)) {
        cs_set_error("cs_liveview_frame_dev: no memory for %d staging rows", nMap);
        return CS_ERR_ALLOC;
    }
    LvArgs A;
    memset(&A, 0, sizeof(A));
    int blocks;
    lv_grid(nMap, blocks, A.rowsPerBlock);
    const int ts = (int)(v->calls % v->trailDepth), publish = frame % v->every == 0, s = (int)(v->published % v->depth);
    A.nCams = v->nCams, A.nMap = nMap, A.frame = frame, A.every = v->every, A.lists = 1, A.publish = publish, A.curCap = v->curCap, A.dynCap = v->dynCap;
    A.mapCount = d_mapCount, A.pointFeat = d_pointFeat, A.mapFlags = d_mapFlags, A.mapPts = d_mapPts, A.R = d_R, A.t = d_t, A.groups = d_groups;
    A.scratch = v->dScratch, A.stageCur = v->dStageCur, A.stageDyn = v->dStageDyn, A.totals = v->dTotals;
    A.dynOut = v->dDyn + (size_t)ts * v->dynCap, A.dynCount = v->dDynCount + ts, A.dynFrame = v->dDynFrame + ts;
    if (publish) {
        A.hdr = (cs_live_header*)(v->dRing + (size_t)s * v->slotBytes);
        A.pts = (cs_live_point*)(v->dRing + (size_t)s * v->slotBytes + sizeof(cs_live_header));
    }
    hipStream_t st = (hipStream_t)hip_stream;
    hipLaunchKernelGGL(k_live_frame, dim3(blocks), dim3(LV_THREADS), 0, st, A);
    CS_CHECK_LAUNCH();
    v->lastFrame = frame, ++v->calls;
    if (publish) {
        CS_HIP(hipEventRecord(v->landed[s], st));
        v->frameOf[s] = frame, ++v->published;
    }
    return CS_OK;
}

extern "C" int cs_liveview_newest(cs_liveview* v) {
    if (!v) return -1;
    if (hipSetDevice(v->device) != hipSuccess) return -1;
    for (long long k = v->published - 1; k >= 0 && k >= v->published - v->depth; --k) {
        const int s = (int)(k % v->depth);
        if (hipEventQuery(v->landed[s]) == hipSuccess) return v->frameOf[s];
    }
    (void)hipGetLastError();   // (hipErrorNotReady is no error of ours)
    return -1;
}

extern "C" int cs_liveview_fetch(cs_liveview* v, int frame, const cs_live_header** header, const cs_live_point** points) {
    if (!v || frame < 0 || !header || !points) {
        cs_set_error("cs_liveview_fetch: bad arguments");
        return CS_ERR_INVALID;
    }
    int s = -1;
    for (int q = 0; q < v->depth; ++q)
        if (v->frameOf[q] == frame) s = q;
    if (s < 0) {
        cs_set_error("cs_liveview_fetch: frame %d is not in the ring (never published, or overwritten; every %d, depth %d)", frame, v->every,
                     v->depth);
        return CS_ERR_INVALID;
    }
    CS_HIP(hipSetDevice(v->device));
    CS_HIP(hipEventSynchronize(v->landed[s]));
    *header = (const cs_live_header*)(v->hRing + (size_t)s * v->slotBytes);
    *points = (const cs_live_point*)(v->hRing + (size_t)s * v->slotBytes + sizeof(cs_live_header));
    return CS_OK;
}

extern "C" int cs_liveview_rings(cs_liveview* v, const unsigned char** h_ring, size_t* slotBytes, const cs_live_dyn** d_entries,
                                 const int** d_counts, const int** d_frames) {
    if (!v) {
        cs_set_error("cs_liveview_rings: null view");
        return CS_ERR_INVALID;
    }
    if (h_ring) *h_ring = v->hRing;
    if (slotBytes) *slotBytes = v->slotBytes;
    if (d_entries) *d_entries = v->dDyn;
    if (d_counts) *d_counts = v->dDynCount;
    if (d_frames) *d_frames = v->dDynFrame;
    return CS_OK;
}

// one frame's dynamic list from the device ring to the host: a copy behind hip_stream and a wait
extern "C" int cs_liveview_dyn_fetch(cs_liveview* v, void* hip_stream, int framesBack, int maxEntries, cs_live_dyn* h_entries, int* count,
                                     int* frame) {
    if (!v || framesBack < 0 || maxEntries < 0 || !count || !frame || (maxEntries > 0 && !h_entries)) {
        cs_set_error("cs_liveview_dyn_fetch: bad arguments");
        return CS_ERR_INVALID;
    }
    if (framesBack >= v->trailDepth || framesBack >= v->calls) {
        cs_set_error("cs_liveview_dyn_fetch: %d frames back is not in the ring (%lld frames stored of %d)", framesBack,
                     v->calls < v->trailDepth ? v->calls : (long long)v->trailDepth, v->trailDepth);
        return CS_ERR_INVALID;
    }
    CS_HIP(hipSetDevice(v->device));
    hipStream_t st = (hipStream_t)hip_stream;
    const int slot = (int)((v->calls - 1 - framesBack) % v->trailDepth);
    CS_HIP(hipMemcpyAsync(count, v->dDynCount + slot, sizeof(int), hipMemcpyDeviceToHost, st));
    CS_HIP(hipMemcpyAsync(frame, v->dDynFrame + slot, sizeof(int), hipMemcpyDeviceToHost, st));
    CS_HIP(hipStreamSynchronize(st));
    const int n = *count < maxEntries ? *count : maxEntries;
    if (n > 0) {
        CS_HIP(hipMemcpyAsync(h_entries, v->dDyn + (size_t)slot * v->dynCap, sizeof(cs_live_dyn) * n, hipMemcpyDeviceToHost, st));
        CS_HIP(hipStreamSynchronize(st));
    }
    return CS_OK;
}

extern "C" int cs_liveview_trails_dev(cs_liveview* v, void* hip_stream, int trjLen, int* d_nTrails, int* d_trailId, int* d_trailLen,
                                      double* d_trailPts) {
    if (!v || trjLen < 0 || !d_nTrails || !d_trailId || !d_trailLen || !d_trailPts) {
        cs_set_error("cs_liveview_trails_dev: bad arguments (null output, trjLen < 0)");
        return CS_ERR_INVALID;
    }
    if (trjLen > v->trailDepth) {
        cs_set_error("cs_liveview_trails_dev: trjLen %d is more than the ring's %d frames", trjLen, v->trailDepth);
        return CS_ERR_INVALID;
    }
    CS_HIP(hipSetDevice(v->device));
    const long long stored = v->calls < v->trailDepth ? v->calls : v->trailDepth;
    LtArgs A;
    A.trjLen = trjLen, A.L = (int)(trjLen < stored ? trjLen : stored);
    A.newest = v->calls ? (int)((v->calls - 1) % v->trailDepth) : 0, A.trailDepth = v->trailDepth, A.dynCap = v->dynCap;
    A.ring = v->dDyn, A.count = v->dDynCount, A.nTrails = d_nTrails, A.trailId = d_trailId, A.trailLen = d_trailLen, A.trailPts = d_trailPts;
    const int blocks = v->dynCap < 1024 ? v->dynCap : 1024;
    hipLaunchKernelGGL(k_live_trails, dim3(blocks), dim3(64), 0, (hipStream_t)hip_stream, A);
    CS_CHECK_LAUNCH();
    return CS_OK;
}

extern "C" int cs_liveview_trails(cs_liveview* v, void* hip_stream, int trjLen, int maxTrails, int* nTrails, int* h_trailId, int* h_trailLen,
                                  double* h_trailPts) {
    if (!v || trjLen < 0 || maxTrails < 0 || !nTrails || (maxTrails > 0 && (!h_trailId || !h_trailLen || !h_trailPts))) {
        cs_set_error("cs_liveview_trails: bad arguments (null output, trjLen < 0)");
        return CS_ERR_INVALID;
    }
    if (trjLen > v->trailDepth) {
        cs_set_error("cs_liveview_trails: trjLen %d is more than the ring's %d frames", trjLen, v->trailDepth);
        return CS_ERR_INVALID;
    }
    CS_HIP(hipSetDevice(v->device));
    if (!v->dTrPts) {   // (sized for the longest trail the ring can give)
        CS_HIP(hipMalloc((void**)&v->dTrN, sizeof(int)));
        CS_HIP(hipMalloc((void**)&v->dTrId, sizeof(int) * v->dynCap));
        CS_HIP(hipMalloc((void**)&v->dTrLen, sizeof(int) * v->dynCap));
        CS_HIP(hipMalloc((void**)&v->dTrPts, sizeof(double) * 3 * (size_t)v->dynCap * v->trailDepth));
    }
    hipStream_t st = (hipStream_t)hip_stream;
    const int rc = cs_liveview_trails_dev(v, hip_stream, trjLen, v->dTrN, v->dTrId, v->dTrLen, v->dTrPts);
    if (rc != CS_OK) return rc;
    CS_HIP(hipMemcpyAsync(nTrails, v->dTrN, sizeof(int), hipMemcpyDeviceToHost, st));
    CS_HIP(hipStreamSynchronize(st));
    const int n = *nTrails < maxTrails ? *nTrails : maxTrails;
    if (n > 0) {
        CS_HIP(hipMemcpyAsync(h_trailId, v->dTrId, sizeof(int) * n, hipMemcpyDeviceToHost, st));
        CS_HIP(hipMemcpyAsync(h_trailLen, v->dTrLen, sizeof(int) * n, hipMemcpyDeviceToHost, st));
        if (trjLen > 0) CS_HIP(hipMemcpyAsync(h_trailPts, v->dTrPts, sizeof(double) * 3 * (size_t)n * trjLen, hipMemcpyDeviceToHost, st));
        CS_HIP(hipStreamSynchronize(st));
    }
    return CS_OK;
}

extern "C" size_t cs_map_counts_scratch_bytes(void) { return sizeof(int) * LV_SCR_INTS; }

extern "C" int cs_map_counts_dev(int device, void* hip_stream, int nCams, int nMap, const int* d_mapCount, const int* d_pointFeat,
                                 const unsigned char* d_mapFlags, cs_map_counts* d_counts, void* d_scratch) {
    if (nCams < 1 || nCams > LV_MAX_CAMS) {
        cs_set_error("cs_map_counts_dev: %d cameras (1..%d)", nCams, LV_MAX_CAMS);
        return CS_ERR_INVALID;
    }
    if (nMap < 0 || !d_pointFeat || !d_counts || !d_scratch) {
        cs_set_error("cs_map_counts_dev: bad arguments (null table, output or scratch, nMap < 0)");
        return CS_ERR_INVALID;
    }
    CS_HIP(hipSetDevice(device));
    LvArgs A;
    memset(&A, 0, sizeof(A));
    int blocks;
    lv_grid(nMap, blocks, A.rowsPerBlock);
    A.nCams = nCams, A.nMap = nMap, A.mapCount = d_mapCount, A.pointFeat = d_pointFeat, A.mapFlags = d_mapFlags, A.counts = d_counts;
    A.scratch = (int*)d_scratch;
    hipLaunchKernelGGL(k_live_frame, dim3(blocks), dim3(LV_THREADS), 0, (hipStream_t)hip_stream, A);
    CS_CHECK_LAUNCH();
    return CS_OK;
}
