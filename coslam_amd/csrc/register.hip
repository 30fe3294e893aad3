// register.hip -- the search step of CoSLAM's map-point registration for all points x all cameras in one launch, gfx950
// (SURVEY.md 8f-2).
//
// Replaces, inside the three registration loops of the reference
//   CoSLAM::curStaticPointRegInGroup        src/app/SL_CoSLAM.cpp:731-757
//   CoSLAM::curDynamicPointRegInGroup       src/app/SL_CoSLAM.cpp:955-980
//   CoSLAM::activeMapPointRegisterInGroup   src/app/SL_CoSLAM.cpp:1118-1145
// the per (map point, camera) statements that are the same in all three -- isAtCameraBack, project, the image test,
// getProjectionCovMat, searchMahaNearestFeatPt (src/app/SL_SingleSLAM.cpp:1141-1164: a serial walk over the camera's
// feature list of the current frame) -- plus the candidate's own term of staticCheckMergability (SL_CoSLAM.cpp:714-729).
// The reference runs them point by point, camera by camera, under the BA mutex: P x C x N distance evaluations on one
// host core per frame (1500 x 8 x 2000 = 24 M).  What the loops do with a candidate afterwards (NCC comparison, the walk
// over the candidate's earlier frames, pointer updates, refineMapPoint, checkUnify) stays with the caller.
//
// Layout: one workgroup per (tile of 64 map points, camera); lane = point, the camera's feature list (the hand-back's SoA
// records x[N], y[N], state[N]) staged in LDS once and walked with broadcast reads by 16 waves, 1/16 of the list each; the
// waves' minima are merged on (distance, slot) -- exactly the serial loop's "strict <, first wins".  The first version ran
// one wave per pair with the lanes striding the list out of L2: 12000 waves x 2000 x 20 B = 480 MB of L1 fills per launch,
// 59 us in the benchmark loop; staging cuts that to 15 MB.  A pair the reference skips (feature of this frame already
// attached, behind the camera, outside the image) only idles its lane.
//
// searchMahaNearestFeatPt scales the inverse covariance by 1 / maxDist and never compares the distance with a threshold:
// the nearest feature in that metric wins however far it is.  Reproduced as is; the scaled distance is returned so the
// caller can gate.  isAtCameraBack / project / getProjectionCovMat / mat22Inv / mahaDist2 are un-vendored LibVisualSLAM:
// definitions in DESIGN.md, same arithmetic order as the test oracle, no FMA contraction.
#include "cs_common.h"
#include "register_rows_dev.h"

#include <cfloat>

#pragma clang fp contract(off)

namespace {


struct RgArgs {
    int nCams, N, W, H, nPass, cam0;   // cameras cam0 .. cam0 + gridDim.y - 1 of the nCams-wide tables
    cs_register_pass pass[2];  // blockIdx.z: the passes of a frame share ONE launch (cs_register_search_passes_dev)
    cs_register_cam cam[RG_MAX_CAMS];
};


// The kernel has to FIT beside the persistent tracker, whose workgroups hold two waves of 160 VGPRs on every SIMD and 128 of a compute
// unit's 160 KB of LDS for as long as its main kernel runs: 192 VGPRs per SIMD lane and 32 KB of LDS are what is left.  8 waves of 96
// VGPRs (two per SIMD) and a 512-feature stage (8 KB + 6 KB of tables) fit; round 3's 16 waves (four per SIMD: 384 VGPRs) with the
// whole list staged (44 KB) did not -- a search that became ready before the tracker's main kernel had retired waited for it.
// Measured in the loop, alternating on one box (profiles/r04_ab_runs.txt): 16 waves / whole list 2141-2148 frames/s, 8 / 1024 2159-2167,
// 8 / 512 2173-2179, 8 / 256 2159, 16 / 512 2134-2141, 4 / 512 2128-2140.
constexpr int RG_WAVES = 8;       // waves per workgroup: each scans 1 / 8 of the staged features for the block's 64 points
constexpr int RG_ROWS = RG_WAVES > 6 ? RG_WAVES : 6;   // rows of the minima table (it first carries the 6 projection values)
constexpr int RG_CHUNK = 512;     // features staged in LDS at a time; the list is scanned chunk by chunk

// One workgroup = 64 map points x one camera.  Lane = point: its projection and scaled inverse covariance live in
// registers.  The camera's feature list is staged in LDS once per workgroup (x, y as doubles; a slot that is not in this
// frame's list is staged as NaN, so its distance compares false and it can never win -- no state test in the loop), and
// every wave walks its share of it with BROADCAST reads: one LDS read serves 64 points.  Per wave the walk is in slot
// order with a strict <, the waves' minima are merged lexicographically on (distance, slot): the serial loop's answer.
// (Round 4 built the alternative -- features binned into 32-pixel cells, a point looks at 3 x 3 cells and falls back to the full scan
// when it cannot prove the answer global: 33 x fewer distance evaluations, bit-identical tables, 18.6 + 10.4 us alone -- and measured it
// in the loop: 2114 / 2118 frames/s against this kernel's 2168 / 2159.  Scattered reads and a second launch cost more next to the tracker
// than 50 M broadcast-fed evaluations.  Deleted; profiles/r04_ab_runs.txt.)
__global__ __launch_bounds__(64 * RG_WAVES) void k_register_search(RgArgs A) {
    extern __shared__ double lds[];
    CS_POSE_STREAM_PRIO();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int c = A.cam0 + blockIdx.y;
    const cs_register_pass& Q = A.pass[blockIdx.z];
    // Q.list: the pass's points are list[0 .. P) (map indices, < 0: no point) -- the tables stay indexed by the MAP index, so a compact
    // list of the frame's current points (cs_register_list_current_dev) costs one workgroup per 64 LISTED points and camera
    const int j = blockIdx.x * 64 + lane;
    if (Q.list && (int)(blockIdx.x * 64) < Q.P && Q.list[blockIdx.x * 64] < 0) return;   // (a compact list: this tile lies behind its end)
    const int p = Q.list ? (j < Q.P ? Q.list[j] : -1) : (j < Q.P ? j : -1);
    const cs_register_cam& C = A.cam[c];
    const int N = A.N;
    const int CH = N < RG_CHUNK ? N : RG_CHUNK;
    double* sx = lds;
    double* sy = lds + CH;
    double* cd = lds + 2 * CH;                        // [RG_ROWS][64]
    int* ci = (int*)(cd + RG_ROWS * 64);              // [RG_WAVES][64]
    const size_t o = (size_t)(p < 0 ? 0 : p) * A.nCams + c;
    int outSlot = -1, outFlags = 0;
    double m0 = 0, m1 = 0, var[4] = {0, 0, 0, 0}, outDist = 0;
    double ivar[4] = {0, 0, 0, 0};
    bool search = false;
    Proj q;
    if (wave == 0 && p >= 0) search = rg_pair_begin(Q, C, o, p, A.W, A.H, q, m0, m1, var, ivar, outSlot);
    if (__syncthreads_or(search)) {
        // the projection and the scaled inverse covariance were worked out by wave 0 only: hand them to the other waves
        double* sq = cd;  // [6][64], overwritten by the minima after the scan
        if (wave == 0) {
            sq[lane] = m0;
            sq[64 + lane] = m1;
#pragma unroll
            for (int k = 0; k < 4; ++k) sq[(2 + k) * 64 + lane] = ivar[k];
        }
        __syncthreads();
        if (wave != 0) {
            m0 = sq[lane];
            m1 = sq[64 + lane];
#pragma unroll
            for (int k = 0; k < 4; ++k) ivar[k] = sq[(2 + k) * 64 + lane];
        }
        // ---- searchMahaNearestFeatPt, SL_SingleSLAM.cpp:1141-1164 ----
        const double* __restrict__ xs = C.xy;
        const double* __restrict__ ys = C.xy + N;
        const int* __restrict__ st = C.state;
        double dMin = DBL_MAX;
        int iMin = 0x7fffffff;
        for (int base = 0; base < N; base += CH) {
            const int n = (N - base) < CH ? (N - base) : CH;
            if (base) __syncthreads();
            for (int i = threadIdx.x; i < n; i += 64 * RG_WAVES) {
                const int s = st[base + i];
                const bool in = (s == 0 || s == 1);
                sx[i] = in ? xs[base + i] : __builtin_nan("");
                sy[i] = in ? ys[base + i] : __builtin_nan("");
            }
            __syncthreads();
            const int per = (n + RG_WAVES - 1) / RG_WAVES;
            const int lo = wave * per, hi = (lo + per) < n ? (lo + per) : n;
            for (int i = lo; i < hi; ++i) {
                const double d = maha_dist2(m0, m1, sx[i], sy[i], ivar);
                if (d < dMin) {
                    dMin = d;
                    iMin = base + i;
                }
            }
        }
        cd[wave * 64 + lane] = dMin;  // (every wave read its copy of sq before the staging barrier above)
        ci[wave * 64 + lane] = iMin;
        __syncthreads();
        if (wave == 0 && search) {
#pragma unroll 4
            for (int w = 1; w < RG_WAVES; ++w) {
                const double d2 = cd[w * 64 + lane];
                const int i2 = ci[w * 64 + lane];
                if (d2 < dMin || (d2 == dMin && i2 < iMin)) {
                    dMin = d2;
                    iMin = i2;
                }
            }
            rg_pair_finish(Q, C, p, N, q, m0, m1, dMin, iMin, outSlot, outFlags, outDist);
        }
    }
    if (wave == 0 && p >= 0) rg_pair_store(Q, o, outSlot, outFlags, outDist, m0, m1, var);
}

// ---- the frame's CURRENT map points as a compact list ------------------------------------------------------------------------------
// CoSLAM::currentMapPointsRegister walks curMapPts: the points with a feature of this frame in at least one camera (mapStateUpdate,
// src/app/SL_CoSLAM.cpp:1176-1194, moves every other point off the list; :734 / :958 ask numVisCam > 0 again) -- wherever they sit
// in the map, the points genNewMapPoints has just appended included.  One workgroup: a point is listed when it lies below the
// live count, is not false (neither registration loop visits a false point) and holds a feature of this frame; the list keeps the
// map's order (the order the reference's walks visit the points in).  list[count .. nMap) = -1; the rows of the points that
// left the list since the previous call get slot = -1 in `slotTable` (nMap x nCams, optional; it starts at -1 everywhere and only
// listed rows are ever written), so that the tables never carry a stale candidate.
__global__ __launch_bounds__(1024) void k_register_list(int nCams, int nMap, const int* __restrict__ mapCount, const int* __restrict__ pointFeat,
                                                        const unsigned char* __restrict__ mapFlags, int* __restrict__ list,
                                                        int* __restrict__ listCount, int* __restrict__ slotTable, int listCap,
                                                        int* __restrict__ overflow) {
    // pass 1, coalesced: thread t looks at the points t, t + 1024, ... (a wave = 64 consecutive rows of pointFeat), the verdicts go into
    // a bitmap in LDS (and the unlisted points' rows of slotTable to -1); pass 2: thread t owns `per` consecutive points of the bitmap
    // (the list keeps the map's order): count, ONE scan over the block, write.  (Earlier forms: 15 rounds of scan over 1024 points,
    // 35 us; a thread reading its own 15 rows of pointFeat, 64 cache lines per wave load, 68 us.)
    __shared__ unsigned long long bits[1024];   // 65536 points
    __shared__ int waveSum[16];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int live = mapCount ? (*mapCount < nMap ? *mapCount : nMap) : nMap;
    const bool vec4 = (nCams & 3) == 0 && (reinterpret_cast<uintptr_t>(pointFeat) & 15) == 0;
    const bool vec4s = (nCams & 3) == 0 && (reinterpret_cast<uintptr_t>(slotTable) & 15) == 0;
    const int oldCount = listCount ? (*listCount < nMap ? (*listCount < 0 ? 0 : *listCount) : nMap) : nMap;   // `list` still holds the previous call's
    for (int w = tid; w < (nMap + 63) / 64; w += 1024) bits[w] = 0ull;
    __syncthreads();
    // (eight trips' loads in flight together: the rows are independent, a trip by itself is one dependent round of memory latency)
    for (int pb = wv * 64; pb < live; pb += 8 * 1024) {
        int4 v0[8], v1[8];
        unsigned char fl[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const int p = pb + 1024 * k + lane;
            v0[k] = v1[k] = make_int4(-1, -1, -1, -1), fl[k] = CS_MAP_FALSE;
            if (p < live) {
                fl[k] = mapFlags ? mapFlags[p] : 0;
                if (vec4 && nCams <= 8) {   // (rows of 4 or 8 ints on a 16-byte boundary: one or two 16-byte loads)
                    const int4* row = reinterpret_cast<const int4*>(pointFeat + (size_t)p * nCams);
                    v0[k] = row[0];
                    if (nCams == 8) v1[k] = row[1];
                }
            }
        }
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const int p0 = pb + 1024 * k, p = p0 + lane;
            if (p0 >= live) break;   // (uniform over the wave)
            bool in = false;
            if (p < live && !(fl[k] & CS_MAP_FALSE)) {
                if (vec4 && nCams <= 8) {
                    in = v0[k].x >= 0 || v0[k].y >= 0 || v0[k].z >= 0 || v0[k].w >= 0 || v1[k].x >= 0 || v1[k].y >= 0 || v1[k].z >= 0 || v1[k].w >= 0;
                } else if (vec4) {
                    const int4* row = reinterpret_cast<const int4*>(pointFeat + (size_t)p * nCams);
                    for (int c = 0; c < nCams / 4; ++c) {
                        const int4 v = row[c];
                        in |= v.x >= 0 || v.y >= 0 || v.z >= 0 || v.w >= 0;
                    }
                } else {
                    for (int c = 0; c < nCams; ++c) in |= pointFeat[(size_t)p * nCams + c] >= 0;
                }
            }
            const unsigned long long b = __builtin_amdgcn_ballot_w64(in);
            if (lane == 0) bits[p0 >> 6] = b;
        }
    }
    __syncthreads();
    // the rows of the points that were on the list a call ago and are not any more lose their candidates (every other unlisted row
    // lost them when it left the list, or never had any: the table starts at -1) -- a few hundred rows instead of the whole map's
    if (slotTable) {
        for (int q = tid; q < oldCount; q += 1024) {
            const int p = list[q];
            if (p < 0 || p >= nMap || ((bits[p >> 6] >> (p & 63)) & 1ull)) continue;
            if (vec4s) {
                int4* row = reinterpret_cast<int4*>(slotTable + (size_t)p * nCams);
                for (int c = 0; c < nCams / 4; ++c) row[c] = make_int4(-1, -1, -1, -1);
            } else {
                for (int c = 0; c < nCams; ++c) slotTable[(size_t)p * nCams + c] = -1;
            }
        }
    }
    __syncthreads();   // (the previous list has been read: it may be overwritten)
    const int per = (nMap + 1023) / 1024;
    const int q0 = tid * per, q1 = (q0 + per) < nMap ? (q0 + per) : nMap;
    int cnt = 0;
    for (int p = q0; p < q1; ++p) cnt += (int)((bits[p >> 6] >> (p & 63)) & 1ull);
    int inc = cnt;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int v = __shfl_up(inc, o, 64);
        if (lane >= o) inc += v;
    }
    if (lane == 63) waveSum[wv] = inc;
    __syncthreads();
    int off = inc - cnt, total = 0;
    for (int w = 0; w < 16; ++w) {
        if (w < wv) off += waveSum[w];
        total += waveSum[w];
    }
    // listCap: the passes behind this list (search, running mergability, merge walk, candidate records) cover its first listCap
    // entries.  A current point beyond the cap is NOT listed this frame: its row of slotTable is cleared, so that the decision -- which
    // visits every point with a feature -- finds no candidate for it instead of an older frame's; *overflow counts such points.
    const int kept = total < listCap ? total : listCap;
    for (int p = q0; p < q1; ++p)
        if ((bits[p >> 6] >> (p & 63)) & 1ull) {
            if (off < listCap) list[off] = p;
            else if (slotTable)
                for (int c = 0; c < nCams; ++c) slotTable[(size_t)p * nCams + c] = -1;
            ++off;
        }
    for (int q = kept + tid; q < nMap; q += 1024) list[q] = -1;
    if (tid == 0 && listCount) *listCount = kept;
    if (tid == 0 && overflow && total > listCap) atomicAdd(overflow, total - listCap);
}

int check_args(const char* who, int nCams, const cs_register_cam* cams, int N, int W, int H, int P, double sigmaSearch,
               double maxDist, double sigmaMerge) {
    if (nCams < 1 || nCams > RG_MAX_CAMS || !cams || N < 1 || W < 1 || H < 1 || P < 0 || !(maxDist > 0) || !(sigmaSearch >= 0) ||
        !(sigmaMerge >= 0)) {
        cs_set_error("%s: bad arguments (1..%d cameras, N >= 1, maxDist > 0)", who, RG_MAX_CAMS);
        return CS_ERR_INVALID;
    }
    return CS_OK;
}

}  // namespace

extern "C" int cs_register_list_current_dev(int device, void* hip_stream, int nCams, int nMap, const int* d_mapCount, const int* d_pointFeat,
                                            const unsigned char* d_mapFlags, int* d_list, int* d_listCount, int* d_slotTable) {
    return cs_register_list_current_cap_dev(device, hip_stream, nCams, nMap, d_mapCount, d_pointFeat, d_mapFlags, d_list, d_listCount, d_slotTable,
                                            nMap, nullptr);
}

extern "C" int cs_register_list_current_cap_dev(int device, void* hip_stream, int nCams, int nMap, const int* d_mapCount, const int* d_pointFeat,
                                                const unsigned char* d_mapFlags, int* d_list, int* d_listCount, int* d_slotTable, int listCap,
                                                int* d_overflow) {
    if (nCams < 1 || nCams > RG_MAX_CAMS || nMap < 0 || nMap > 65536 || listCap < 0 || (nMap > 0 && (!d_pointFeat || !d_list))) {
        cs_set_error("cs_register_list_current_dev: bad arguments (at most 65536 map points)");
        return CS_ERR_INVALID;
    }
    if (nMap == 0) return CS_OK;
    CS_HIP(hipSetDevice(device));
    hipLaunchKernelGGL(k_register_list, dim3(1), dim3(1024), 0, (hipStream_t)hip_stream, nCams, nMap, d_mapCount, d_pointFeat, d_mapFlags, d_list,
                       d_listCount, d_slotTable, listCap < nMap ? listCap : nMap, d_overflow);
    CS_CHECK_LAUNCH();
    return CS_OK;
}

extern "C" int cs_register_search_passes_dev(int device, void* hip_stream, int nCams, const cs_register_cam* cams, int N, int W, int H,
                                             int nPass, const cs_register_pass* passes) {
    return cs_register_search_passes_range_dev(device, hip_stream, nCams, 0, nCams, cams, N, W, H, nPass, passes);
}

// cameras cam0 .. cam0 + nCamsRun - 1 only: their columns of the nCams-wide tables (a rank that holds every camera's records but
// searches only for the cameras it owns)
extern "C" int cs_register_search_passes_range_dev(int device, void* hip_stream, int nCams, int cam0, int nCamsRun, const cs_register_cam* cams,
                                                   int N, int W, int H, int nPass, const cs_register_pass* passes) {
    if (cam0 < 0 || nCamsRun < 0 || cam0 + nCamsRun > nCams) {
        cs_set_error("cs_register_search_passes_range_dev: camera range %d + %d of %d", cam0, nCamsRun, nCams);
        return CS_ERR_INVALID;
    }
    if (nPass < 1 || nPass > 2 || !passes) {
        cs_set_error("cs_register_search_passes_dev: 1 or 2 passes");
        return CS_ERR_INVALID;
    }
    RgArgs A;
    memset(&A, 0, sizeof(A));
    A.nCams = nCams, A.N = N, A.W = W, A.H = H, A.nPass = nPass, A.cam0 = cam0;
    int maxP = 0;
    for (int k = 0; k < nPass; ++k) {
        const cs_register_pass& q = passes[k];
        int rc = check_args("cs_register_search_passes_dev", nCams, cams, N, W, H, q.P, q.sigmaSearch, q.maxDist, q.sigmaMerge);
        if (rc != CS_OK) return rc;
        if (q.P > 0 && (!q.M || !q.cov || !q.pointFeat || !q.slot || !q.m || !q.var || !q.dist || !q.flags)) {
            cs_set_error("cs_register_search_passes_dev: null pointer in pass %d", k);
            return CS_ERR_INVALID;
        }
        if (q.mapFlags && !(q.maxDistDynamic > 0)) {
            cs_set_error("cs_register_search_passes_dev: pass %d has mapFlags but maxDistDynamic <= 0", k);
            return CS_ERR_INVALID;
        }
        A.pass[k] = q;
        if (q.P > maxP) maxP = q.P;
    }
    if (maxP == 0 || nCamsRun == 0) return CS_OK;
    for (int c = cam0; c < cam0 + nCamsRun; ++c) {
        const cs_register_cam& q = cams[c];
        if (!q.K || !q.R || !q.t || !q.xy || !q.state || !q.slot2map) {
            cs_set_error("cs_register_search_passes_dev: null pointer in camera %d", c);
            return CS_ERR_INVALID;
        }
        A.cam[c] = q;
    }
    CS_HIP(hipSetDevice(device));
    const int CH = N < RG_CHUNK ? N : RG_CHUNK;
    const size_t ldsBytes = (size_t)2 * CH * sizeof(double) + (size_t)RG_ROWS * 64 * sizeof(double) + (size_t)RG_WAVES * 64 * sizeof(int);
    hipLaunchKernelGGL(k_register_search, dim3((unsigned)((maxP + 63) / 64), (unsigned)nCamsRun, (unsigned)nPass), dim3(64 * RG_WAVES), ldsBytes,
                       (hipStream_t)hip_stream, A);
    CS_CHECK_LAUNCH();
    return CS_OK;
}

extern "C" int cs_register_search_dev(int device, void* hip_stream, int nCams, const cs_register_cam* cams, int N, int W, int H,
                                      int P, const double* d_M, const double* d_cov, const int* d_pointFeat, double sigmaSearch,
                                      double maxDist, double sigmaMerge, int* d_slot, double* d_m, double* d_var, double* d_dist,
                                      int* d_flags) {
    int rc = check_args("cs_register_search_dev", nCams, cams, N, W, H, P, sigmaSearch, maxDist, sigmaMerge);
    if (rc != CS_OK) return rc;
    if (P == 0) return CS_OK;
    if (!d_M || !d_cov || !d_pointFeat || !d_slot || !d_m || !d_var || !d_dist || !d_flags) {
        cs_set_error("cs_register_search_dev: null pointer");
        return CS_ERR_INVALID;
    }
    cs_register_pass q;
    memset(&q, 0, sizeof(q));
    q.P = P, q.sigmaSearch = sigmaSearch, q.maxDist = maxDist, q.sigmaMerge = sigmaMerge;
    q.M = d_M, q.cov = d_cov, q.pointFeat = d_pointFeat, q.slot = d_slot, q.m = d_m, q.var = d_var, q.dist = d_dist, q.flags = d_flags;
    return cs_register_search_passes_dev(device, hip_stream, nCams, cams, N, W, H, 1, &q);
}

namespace {

// ---- the decision behind the current-static search: who attaches which feature -------------------------------------------------------
// CoSLAM::curStaticPointsRegInGroup / curStaticPointRegInGroup with bMerge == false (src/app/SL_CoSLAM.cpp:854-898, 731-830) walk the
// points one after the other: for every camera o, the certainly static points with a feature of this frame in o, in map order; each
// walks the cameras in order and attaches the nearest feature where that is unmapped and mergeable, and STOPS at the first feature
// that already carries a map point (:789-790) -- including one an earlier point has just taken.  The only coupling between the walks
// is that: a feature belongs to the FIRST walk step that reaches it unmapped and can take it.  With step order
// ((first camera in which the point has a feature) x P + point) x C + camera, owner[feature] = the smallest order among the steps
// that (a) are reached -- no earlier camera of the same walk met a feature mapped on arrival: mapped before the pass, or owned by a
// step of smaller order -- and (b) may attach.  That is a recursion along a total order, so it has ONE solution, the sequential
// result; Jacobi sweeps (every walk re-evaluated against the previous sweep's owners) reach it in as many sweeps as the longest
// chain of walks cutting each other short -- two or three here.  A fixed number of sweeps as launches over all points (k_decide_sweep,
// the owners in a caller-supplied scratch), or -- what the frame loops run -- as many as it takes, in the launch that builds the walks'
// tables, among the few walks that can claim a feature at all (rd_resolve).
// A point's later visits (it appears once per camera in which it has a feature) find what its first visit left and change nothing.
struct RdArgs {
    int nCams, N, P, mapBase, nSweeps, onlyCam, kinds;
    const int* slot;                 // [P][nCams] the search's candidates
    const int* flags;                // [P][nCams] bit 1: the candidate is dynamic
    const unsigned char* mergeable;  // [P][nCams] 1: mergeable over the whole track
    const unsigned char* mapFlags;   // [P] CS_MAP_* of the pass's points
    int* pointFeat;                  // [P][nCams] in / out
    int* slot2map[RD_MAX_CAMS];      // [N] per camera, in / out
    unsigned char* attached;         // [P][nCams] out
    unsigned char* regged;           // [P] out: refineMapPoint is due (:889-893)
    int* code;                       // scratch [nCams][P]: the walk's view of (point, camera), see RD_* below
    int* base;                       // scratch [P]: order of the point's walk (x nCams), -1: the point is not visited
    int* owner[3];                   // scratch 3 x [nCams * N]: the sweeps rotate through them
    int* counts;                     // [4] out: features attached, points regged, sweeps, converged
    int* unconverged;                // the scratch's last word: the NUMBER of calls whose sweeps did not settle (never cleared here)
    int* timeouts;                   // the word before it: calls that ended on a time-out.  Nothing here waits for anything any more: it
                                     // stays 0 (both frame loops read it)
    int* callFlag;                   // the word before it: this call has been counted (k_decide_sweep)
    int* ticket;                     // the scratch's FIRST word: workgroups of the self-settling launch that have arrived (0 between calls)
    int* nActive;                    // the word behind it: walks on the active list (0 between calls)
    int* active;                     // scratch [P]: the points whose walk can claim a feature (the self-settling launch)
    // the second visits' first list built by the walks themselves (cs_register_decide_kinds_rounds_dev; null: not asked for): a point that
    // registered and holds a feature in a later camera's loop appends itself -- what k_revisit_list(firstRound) would find
    int* rvLists;                    // [nRounds][rvCap]: cleared to -1 by the launch's prepare part, list 0 filled by its resolver
    int* rvCounts;                   // [nRounds]: cleared; [0] = points appended (may exceed rvCap: the rest is not visited again)
    int rvCap, nRounds;
    int* visitLoop;                  // [P]: the loop of a registered point's visit
    int* nextLoop;                   // [P]: the loop of its next visit
};
constexpr int RD_MAX_SWEEPS = 64;

constexpr int RD_THREADS = 256;
// the resolver's owners in LDS: open addressing on the feature, at most half full (else the owner arrays of the scratch, through L2)
constexpr int RD_LDS_BITS = 10, RD_LDS_CELLS = 1 << RD_LDS_BITS, RD_LDS_ENTRIES = RD_LDS_CELLS / 2;

// ---- the resolver of the self-settling launch: the ACTIVE walks among themselves ---------------------------------------------------------
// A walk influences another only by claiming a feature, and it can only claim a candidate that is unmapped and mergeable with no candidate
// mapped on arrival in front of it.  Every other walk claims nothing and attaches nothing whatever the owners say: the sweeps over the
// active walks alone pass through the same owners, sweep for sweep, as the sweeps over all walks, and end on the same (unique) fixed point.
// A listed walk's codes, cut where the walk ends whatever the owners say (a candidate mapped before the pass): what is left are its
// unmapped candidates, the only features whose owners it reads or claims.  p < 0: no row.
// owner array k mod 3 (selected, not indexed: the arguments then stay in registers -- no private segment)
__device__ __forceinline__ int* rd_owner(const RdArgs& A, int k) {
    const int r = k % 3;
    return r == 0 ? A.owner[0] : (r == 1 ? A.owner[1] : A.owner[2]);
}
template <int MC>
__device__ __forceinline__ void rd_row_load(const RdArgs& A, int p, int (&code)[MC], int& base) {
    base = p >= 0 ? rd_ld(A.base + p) : -1;
#pragma unroll
    for (int i = 0; i < MC; ++i) code[i] = (p >= 0 && i < A.nCams) ? rd_ld(A.code + (size_t)i * A.P + p) : -1;   // (independent loads)
    bool go = base >= 0;
#pragma unroll
    for (int i = 0; i < MC; ++i) {
        if (go && code[i] >= 0 && (code[i] & RD_INIT_MAPPED)) go = false;
        if (!go) code[i] = -1;
    }
}
// the owners in `fin` are final (or the best the sweeps reached): attach (k_decide_sweep's mode 1), and the second visits' first list.
// The low bits of a code index `fin`: the feature itself, or (keys != null) the cell of the LDS table that holds it.
template <int MC>
__device__ __forceinline__ void rd_row_attach(const RdArgs& A, int p, const int (&code)[MC], int base, const int* fin, const int* keys) {
    if (base < 0) return;
    const int C = A.nCams;
    bool go = true, reg = false;
    int nAtt = 0;
#pragma unroll
    for (int i = 0; i < MC; ++i) {
        if (go && code[i] >= 0) {
            const int ord = base + i, cell = code[i] & RD_FEAT, own = rd_ld(fin + cell);
            if (own < ord) {
                go = false;                                    // mapped on arrival: the walk ends (:789-790)
            } else if ((code[i] & RD_CAN_MERGE) && own == ord) {
                const int s2 = (keys ? keys[cell] : cell) - i * A.N;
                A.slot2map[i][s2] = A.mapBase + p;             // the feature and its predecessors on the track (:771-775): slot2map is per track
                A.pointFeat[(size_t)p * C + i] = s2;            // MapPoint::addFeature
                A.attached[(size_t)p * C + i] = 1;
                reg = true, ++nAtt;
            }
        }
    }
    if (reg) {
        A.regged[p] = 1;
        if (A.counts) atomicAdd(A.counts, nAtt), atomicAdd(A.counts + 1, 1);
        if (A.rvLists && A.onlyCam < 0) {   // k_revisit_list's first round, by the walk itself
            const int last = (base / C) / A.P;   // the loop of this visit: the first camera that held a feature before the pass (the prepare part)
            A.visitLoop[p] = last;
            int b = -1;
            for (int c = C - 1; c > last; --c)
                if (A.pointFeat[(size_t)p * C + c] >= 0) b = c;
            if (b >= 0) {
                const int q = atomicAdd(A.rvCounts, 1);
                if (q < A.rvCap) A.rvLists[q] = p, A.nextLoop[p] = b;
                else atomicAdd(A.rvCounts + A.nRounds, 1);   // (never cleared here: the points beyond the lists over the run)
            }
        }
    }
}
// ONE workgroup, n > 0 listed walks: Jacobi sweeps among them (rv_row_*: the rounds' sweeps), workgroup barriers between the steps, until a
// sweep changes no owner or RD_MAX_SWEEPS have run; then the attach.  Few walks (the usual frame): a thread per walk, its codes in
// registers, the owners in an LDS table keyed by the feature.  A list longer than the workgroup, or one whose candidates would fill the
// table beyond a half (the bootstrap frame): in turns, the codes read again in every step, the owners in the scratch -- only the listed
// walks' candidates are cleared, read or claimed there, so what an earlier call of any shape left in those arrays does not matter.
template <int MC>
__device__ __forceinline__ void rd_resolve(const RdArgs& A, int n, int* sKey, int* sOwn) {
    __shared__ int sChanged;
    const int tid = threadIdx.x;
    int code[MC], base = -1, k = 0;
    bool settled = false;
    if (n <= RD_THREADS && n * A.nCams <= RD_LDS_ENTRIES) {   // (uniform)
        for (int c = tid; c < RD_LDS_CELLS; c += RD_THREADS)
            sKey[c] = -1, sOwn[c] = RD_INF, sOwn[RD_LDS_CELLS + c] = RD_INF, sOwn[2 * RD_LDS_CELLS + c] = RD_INF;
        const int p = tid < n ? rd_ld(A.active + tid) : -1;
        rd_row_load<MC>(A, p, code, base);
        __syncthreads();
#pragma unroll
        for (int i = 0; i < MC; ++i) {
            if (code[i] < 0) continue;
            const int f = code[i] & RD_FEAT;
            unsigned h = ((unsigned)f * 2654435761u) >> (32 - RD_LDS_BITS);
            for (;;) {   // (ends: the table is never more than half full)
                const int old = atomicCAS(&sKey[h], -1, f);
                if (old == -1 || old == f) break;
                h = (h + 1) & (RD_LDS_CELLS - 1);
            }
            code[i] = (code[i] & ~RD_FEAT) | (int)h;
        }
        __syncthreads();
        const int* fin = sOwn;
        for (; k < RD_MAX_SWEEPS;) {
            const int* prev = sOwn + (k % 3) * RD_LDS_CELLS;
            int* next = sOwn + ((k + 1) % 3) * RD_LDS_CELLS;
            int* clear = sOwn + ((k + 2) % 3) * RD_LDS_CELLS;
            if (tid == 0) sChanged = 0;
            rv_row_clear<MC>(code, base, clear);
            __syncthreads();
            rv_row_claim<MC>(code, base, prev, next);
            __syncthreads();
            if (rv_row_changed<MC>(code, base, prev, next)) sChanged = 1;
            __syncthreads();
            fin = next, ++k;
            const int chg = sChanged;
            __syncthreads();
            if (!chg) {
                settled = true;
                break;
            }
        }
        if (p >= 0) rd_row_attach<MC>(A, p, code, base, fin, sKey);
    } else {
        for (int j = tid; j < n; j += RD_THREADS) {
            rd_row_load<MC>(A, rd_ld(A.active + j), code, base);
#pragma unroll
            for (int i = 0; i < MC; ++i)
                if (code[i] >= 0) rd_st(A.owner[0] + (code[i] & RD_FEAT), RD_INF), rd_st(A.owner[1] + (code[i] & RD_FEAT), RD_INF), rd_st(A.owner[2] + (code[i] & RD_FEAT), RD_INF);
        }
        __syncthreads();
        const int* fin = A.owner[0];
        for (; k < RD_MAX_SWEEPS;) {
            const int* prev = rd_owner(A, k);
            int* next = rd_owner(A, k + 1);
            int* clear = rd_owner(A, k + 2);
            if (tid == 0) sChanged = 0;
            for (int j = tid; j < n; j += RD_THREADS) {
                rd_row_load<MC>(A, rd_ld(A.active + j), code, base);
                rv_row_clear<MC>(code, base, clear);
            }
            __syncthreads();
            for (int j = tid; j < n; j += RD_THREADS) {
                rd_row_load<MC>(A, rd_ld(A.active + j), code, base);
                rv_row_claim<MC>(code, base, prev, next);
            }
            __syncthreads();
            int ch = 0;
            for (int j = tid; j < n; j += RD_THREADS) {
                rd_row_load<MC>(A, rd_ld(A.active + j), code, base);
                ch |= rv_row_changed<MC>(code, base, prev, next);
            }
            if (ch) sChanged = 1;
            __syncthreads();
            fin = next, ++k;
            const int chg = sChanged;
            __syncthreads();
            if (!chg) {
                settled = true;
                break;
            }
        }
        for (int j = tid; j < n; j += RD_THREADS) {
            const int p = rd_ld(A.active + j);
            rd_row_load<MC>(A, p, code, base);
            rd_row_attach<MC>(A, p, code, base, fin, nullptr);
        }
    }
    if (tid == 0) {
        if (A.counts) A.counts[2] = k, A.counts[3] = settled ? 1 : 0;
        if (!settled) atomicAdd(A.unconverged, 1);
    }
}

// entry-parallel (coalesced over the P x nCams tables): what every walk will see of (point, camera).  A workgroup takes WHOLE points
// (RD_THREADS / nCams of them: a point's entries are nCams consecutive threads of one workgroup, whatever nCams is).
// nSweeps > 0: the owners start at "nobody" for the sweep launches that follow.
// nSweeps == 0, the self-settling form, ONE launch: the first entry of a point also decides from the workgroup's codes whether its walk
// is ACTIVE (rd_resolve) and appends it to the scratch's list; the workgroup then waits for its (write-through) stores and draws a
// ticket, one relaxed atomic; the workgroup that draws the last one resolves the list -- nobody waits for anybody, nothing has to be co-resident, and
// on a frame without an active walk that is all.  ticket and nActive are left at 0 for the next call (the scratch arrives zeroed, as
// its sticky last word needs it to): they are the scratch's first words, where a call of any other shape finds them too.
template <int MC>
__global__ __launch_bounds__(RD_THREADS) void k_decide_prepare(RdArgs A) {
    __shared__ int sCode[RD_THREADS];
    __shared__ int sKey[RD_LDS_CELLS], sOwn[3 * RD_LDS_CELLS];
    __shared__ int sCount, sFirst, sLast;
    const int tid = threadIdx.x, C = A.nCams, nFeat = C * A.N, ppb = RD_THREADS / C;
    const int g = blockIdx.x * RD_THREADS + tid, stride = gridDim.x * RD_THREADS;
    const bool settle = A.nSweeps == 0;
    if (!settle)
        for (int f = g; f < nFeat; f += stride) A.owner[0][f] = RD_INF, A.owner[1][f] = RD_INF, A.owner[2][f] = RD_INF;
    // Everything the resolver reads, or writes again, is stored WRITE-THROUGH (agent-scope stores: rd_st, rd_st8): it is in memory when
    // the workgroup draws its ticket, with no release fence -- that would write back every dirty line of the XCD's L2, the tracker's too,
    // once per workgroup (the launch took 18 us that way on a frame without an active walk, 11 us more than these tables cost).
    // (sweeps: the resolver's count; 2 where it has nothing to do -- converged: cleared when not)
    if (g < 4 && A.counts) rd_st(A.counts + g, g == 2 ? (settle ? 2 : A.nSweeps) : (g == 3 ? 1 : 0));
    if (g == 0) *A.callFlag = 0;
    if (A.rvLists) {
        for (int f = g; f < A.nRounds * A.rvCap; f += stride) rd_st(A.rvLists + f, -1);
        if (g < A.nRounds) rd_st(A.rvCounts + g, 0);
    }
    const int pl = tid / C, i = tid - pl * C, p = blockIdx.x * ppb + pl;
    const bool live = pl < ppb && p < A.P;
    int code = -1, base = -1;
    if (live) {
        const size_t k = (size_t)p * C + i;
        rd_st8(A.attached + k, 0);
        if (i == 0) rd_st8(A.regged + p, 0);
        // the point's kind: 0 certainly static, 1 certainly dynamic (its walk takes DYNAMIC features only, :981), -1 not visited
        const unsigned char fl = A.mapFlags[p] & (CS_MAP_DYNAMIC | CS_MAP_FALSE | CS_MAP_UNCERTAIN);
        const int kind = (fl == 0 && (A.kinds & 1)) ? 0 : ((fl == CS_MAP_DYNAMIC && (A.kinds & 2)) ? 1 : -1);
        if (A.pointFeat[k] < 0 && kind >= 0) {   // (else :736-737: the point has a feature of this frame there)
            const int s = A.slot[k];
            if (s >= 0 && s < A.N && ((A.flags[k] >> 1) & 1) == kind) {   // (else: nothing found / a feature of the other type, :757 / :981)
                code = i * A.N + s;
                if (A.slot2map[i][s] >= 0) code |= RD_INIT_MAPPED;
                if (A.mergeable[k] == 1) code |= RD_CAN_MERGE;
            }
        }
        rd_st(A.code + (size_t)i * A.P + p, code);
        if (i == 0) {   // the order of the point's walk = ((first camera in which it has a feature of this frame) x P + point) x nCams
            int ofirst = -1;
            for (int q = C - 1; q >= 0; --q)
                if (A.pointFeat[(size_t)p * C + q] >= 0) ofirst = q;
            // onlyCam >= 0: ONE camera's loop of the reference (:864-869): the points with a feature of this frame in that camera, map order
            if (A.onlyCam >= 0) ofirst = A.pointFeat[(size_t)p * C + A.onlyCam] >= 0 ? 0 : -1;
            base = (ofirst >= 0 && kind >= 0) ? (ofirst * A.P + p) * C : -1;
            rd_st(A.base + p, base);
        }
    }
    if (!settle) return;   // (uniform)
    // ---- the active walks of this workgroup's points, appended to the list
    sCode[tid] = code;
    if (tid == 0) sCount = 0;
    __syncthreads();
    bool act = false;
    if (base >= 0) {   // (the point's first entry; its walk, on the codes alone: does it reach a candidate it may take?)
        for (int q = 0; q < C; ++q) {
            const int c = sCode[tid + q];
            if (c < 0) continue;
            if (c & RD_INIT_MAPPED) break;
            if (c & RD_CAN_MERGE) {
                act = true;
                break;
            }
        }
    }
    if (__syncthreads_or(act)) {   // (uniform; the usual workgroup has none)
        const int at = act ? atomicAdd(&sCount, 1) : 0;
        __syncthreads();
        if (tid == 0) sFirst = atomicAdd(A.nActive, sCount);
        __syncthreads();
        if (act && sFirst >= 0 && sFirst + at < A.P) rd_st(A.active + sFirst + at, p);   // (in bounds by construction: the count starts at 0)
    }
    // ---- every wave's stores are in memory; draw a ticket
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (tid == 0) sLast = __hip_atomic_fetch_add(A.ticket, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == (int)gridDim.x - 1;
    __syncthreads();
    if (!sLast) return;   // (uniform)
    // ---- the last workgroup to arrive: every other one's tables, clears and list entries are in memory.  The resolver reads them past
    // its caches (rd_ld); the acquire is for whatever else it loads
    const int n = min(rd_ld(A.nActive), A.P);   // (never beyond the list, whatever a scratch that did not arrive zeroed holds)
    if (n > 0) {
        if (tid == 0) {
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
        __syncthreads();
        rd_resolve<MC>(A, n, sKey, sOwn);
    }
    __syncthreads();
    if (tid == 0) rd_st(A.ticket, 0), rd_st(A.nActive, 0);
}
// one Jacobi sweep, thread per point: its walk against the owners of the previous sweep (prev), claims into next; `clear` is the
// buffer the FOLLOWING sweep will claim into.  mode 1: the owners in prev are final -- attach instead of claiming.
__global__ __launch_bounds__(256) void k_decide_sweep(RdArgs A, const int* __restrict__ prev, int* __restrict__ next, int* __restrict__ clear,
                                                      const int* __restrict__ prev2, int mode) {
    const int p = blockIdx.x * 256 + threadIdx.x, C = A.nCams, nFeat = C * A.N;
    if (clear)
        for (int f = p; f < nFeat; f += gridDim.x * 256) clear[f] = RD_INF;
    if (mode == 1 && prev2) {   // converged: the last two sweeps agree on every owner
        int ch = 0;
        for (int f = p; f < nFeat; f += gridDim.x * 256) ch |= prev[f] != prev2[f];
        if (ch) {
            if (A.counts) A.counts[3] = 0;
            if (atomicExch(A.callFlag, 1) == 0) atomicAdd(A.unconverged, 1);
        }
    }
    if (p >= A.P) return;
    const int base = A.base[p];
    if (base < 0) return;
    int code[RD_MAX_CAMS], own[RD_MAX_CAMS];
#pragma unroll
    for (int i = 0; i < RD_MAX_CAMS; ++i) code[i] = i < C ? A.code[(size_t)i * A.P + p] : -1;
#pragma unroll
    for (int i = 0; i < RD_MAX_CAMS; ++i) own[i] = code[i] >= 0 ? prev[code[i] & RD_FEAT] : RD_INF;   // (independent loads)
    bool go = true, reg = false;
    int nAtt = 0;
#pragma unroll
    for (int i = 0; i < RD_MAX_CAMS; ++i) {
        if (go && code[i] >= 0) {
            const int ord = base + i, f = code[i] & RD_FEAT;
            if ((code[i] & RD_INIT_MAPPED) || own[i] < ord) {
                go = false;                                    // mapped on arrival: the walk ends (:789-790)
            } else if (code[i] & RD_CAN_MERGE) {
                if (mode == 0) {
                    atomicMin(&next[f], ord);                  // it takes the feature unless an earlier step does
                } else if (own[i] == ord) {
                    const int s = f - i * A.N;
                    A.slot2map[i][s] = A.mapBase + p;          // the feature and its predecessors on the track (:771-775): slot2map is per track
                    A.pointFeat[(size_t)p * C + i] = s;         // MapPoint::addFeature
                    A.attached[(size_t)p * C + i] = 1;
                    reg = true, ++nAtt;
                }
            }
        }
    }
    if (mode == 1 && reg) {
        A.regged[p] = 1;
        if (A.counts) atomicAdd(A.counts, nAtt), atomicAdd(A.counts + 1, 1);
    }
}

// ---- the SECOND VISITS of the reference's order (round 6) -----------------------------------------------------------------------------
// CoSLAM::curStaticPointsRegInGroup builds every camera's visiting list afresh (src/app/SL_CoSLAM.cpp:864-869) and refines the points that
// gained a feature at the end of every camera's loop (:889-893): a point that registers in camera a's loop is visited AGAIN in the loop of
// every later camera b in which it holds a feature of this frame -- the one it has just gained included -- projected with its refined
// position.  A later visit of a point that did NOT register changes nothing (same position, same candidates, and a candidate can only have
// gone from unmapped to mapped since, which ends a walk earlier): the single pass above is the reference's run up to the second visits of
// the points it registered.  Those are played here, in rounds: round r visits the points that registered in round r - 1 (round 0 = the
// single pass) in their next loop -- behind a search and a mergability pass over JUST those points at their refined positions -- and a
// refine of the ones that registered again follows.  One workgroup, a thread per listed point; the visits of a round are ordered among
// themselves like all walks ((loop x P + point) x C + camera, Jacobi sweeps over the features they compete for).
// What a round cannot do is take back what a LATER-ordered visit of the single pass did with a feature this visit would have reached
// first: such a frame is counted (conflicts) and left as the single pass decided.  tools/r06_exact_vs_single.py measures what remains.
struct RvListArgs {
    int nCams, P, cap, firstRound;
    const int* pointFeat;              // [P][nCams]
    const unsigned char* attached;     // [P][nCams]: attached in THIS frame (the single pass's and the rounds' so far)
    unsigned char* regIn;              // [P]: registered in the previous round (read; cleared unless keepIn)
    int keepIn;
    unsigned char* regOutClear;        // [P] or null: the array this round's walks will mark -- cleared here (it may hold an earlier frame's marks)
    int* visitLoop;                    // [P]: the loop of the point's latest registering visit
    int* nextLoop;                     // [P]: the loop of the visit listed here
    int* list;                         // [cap] out, padded with -1
    int* counts;                       // [4]: listed, overflow (points beyond cap), -, -
};
__global__ __launch_bounds__(1024) void k_revisit_list(RvListArgs A) {
    __shared__ int sCount;
    const int tid = threadIdx.x, C = A.nCams;
    if (tid == 0) sCount = 0;
    __syncthreads();
    for (int p = tid; p < A.P; p += 1024) {
        if (A.regOutClear) A.regOutClear[p] = 0;
        if (!A.regIn[p]) continue;
        if (!A.keepIn) A.regIn[p] = 0;
        int last;
        if (A.firstRound) {   // the loop of its first visit: the first camera that held a feature of this frame BEFORE the pass attached any
            last = -1;
            for (int c = C - 1; c >= 0; --c)
                if (A.pointFeat[(size_t)p * C + c] >= 0 && !A.attached[(size_t)p * C + c]) last = c;
            A.visitLoop[p] = last;
        } else {
            last = A.visitLoop[p];
        }
        if (last < 0) continue;
        int b = -1;
        for (int c = C - 1; c > last; --c)
            if (A.pointFeat[(size_t)p * C + c] >= 0) b = c;
        if (b < 0) continue;   // no later loop holds the point: it is not visited again
        const int k = atomicAdd(&sCount, 1);
        if (k < A.cap) A.list[k] = p, A.nextLoop[p] = b;
    }
    __syncthreads();
    const int n = sCount < A.cap ? sCount : A.cap;
    for (int k = n + tid; k < A.cap; k += 1024) A.list[k] = -1;
    if (tid == 0 && A.counts) {
        A.counts[0] = n;
        if (sCount > A.cap) atomicAdd(A.counts + 1, sCount - A.cap);
    }
}

template <int MC>
__global__ __launch_bounds__(1024) void k_revisit_decide(RvArgs A) {
    if (A.listCount && *A.listCount == 0) return;   // (uniform: before any barrier)
    rv_decide_rows<MC>(A, rv_round_of(A));
}

}  // namespace

extern "C" int cs_register_revisit_list_dev(int device, void* hip_stream, int nCams, int P, int cap, int firstRound, const int* d_pointFeat,
                                            const unsigned char* d_attached, unsigned char* d_regIn, int keepIn, unsigned char* d_regOutClear,
                                            int* d_visitLoop, int* d_nextLoop, int* d_list, int* d_counts) {
    if (nCams < 1 || nCams > RD_MAX_CAMS || P < 1 || cap < 1 || cap > RV_MAX_ROWS || !d_pointFeat || !d_attached || !d_regIn || d_regOutClear == d_regIn || !d_visitLoop || !d_nextLoop ||
        !d_list) {
        cs_set_error("cs_register_revisit_list_dev: bad arguments (1..%d cameras, 1..%d rows)", RD_MAX_CAMS, RV_MAX_ROWS);
        return CS_ERR_INVALID;
    }
    RvListArgs A;
    A.nCams = nCams, A.P = P, A.cap = cap, A.firstRound = firstRound ? 1 : 0, A.pointFeat = d_pointFeat, A.attached = d_attached;
    A.regIn = d_regIn, A.keepIn = keepIn ? 1 : 0, A.regOutClear = d_regOutClear, A.visitLoop = d_visitLoop, A.nextLoop = d_nextLoop, A.list = d_list, A.counts = d_counts;
    CS_HIP(hipSetDevice(device));
    hipLaunchKernelGGL(k_revisit_list, dim3(1), dim3(1024), 0, (hipStream_t)hip_stream, A);
    CS_CHECK_LAUNCH();
    return CS_OK;
}

extern "C" int cs_register_revisit_decide_dev(int device, void* hip_stream, int nCams, int N, int P, int cap, int mapBase, int kinds, const int* d_list,
                                              const int* d_nextLoop, int* d_visitLoop, const int* d_slot, const int* d_flags,
                                              const unsigned char* d_mergeable, const unsigned char* d_mapFlags, int* d_pointFeat,
                                              int* const* d_slot2map, unsigned char* d_attached, unsigned char* d_regOut, void* d_decideScratch,
                                              const int* d_curList, const int* d_curCount, int curCap, int* d_counts, const int* d_listCount) {
    return cs_register_revisit_decide_next_dev(device, hip_stream, nCams, N, P, cap, mapBase, kinds, d_list, (int*)d_nextLoop, d_visitLoop, d_slot, d_flags,
                                               d_mergeable, d_mapFlags, d_pointFeat, d_slot2map, d_attached, d_regOut, d_decideScratch, d_curList, d_curCount,
                                               curCap, d_counts, d_listCount, nullptr, nullptr, nullptr);
}

extern "C" int cs_register_revisit_decide_next_dev(int device, void* hip_stream, int nCams, int N, int P, int cap, int mapBase, int kinds, const int* d_list,
                                                   int* d_nextLoop, int* d_visitLoop, const int* d_slot, const int* d_flags,
                                                   const unsigned char* d_mergeable, const unsigned char* d_mapFlags, int* d_pointFeat,
                                                   int* const* d_slot2map, unsigned char* d_attached, unsigned char* d_regOut, void* d_decideScratch,
                                                   const int* d_curList, const int* d_curCount, int curCap, int* d_counts, const int* d_listCount,
                                                   int* d_nextList, int* d_nextCount, int* d_overflow) {
    if ((d_nextList != nullptr) != (d_nextCount != nullptr)) {
        cs_set_error("cs_register_revisit_decide_next_dev: the next round's list and its count go together");
        return CS_ERR_INVALID;
    }
    if (nCams < 1 || nCams > RD_MAX_CAMS || N < 1 || P < 1 || cap < 1 || cap > RV_MAX_ROWS || kinds < 1 || kinds > 3 || !d_list ||
        (long long)nCams * N > RD_FEAT || (long long)nCams * P * nCams > 0x7fffffffLL) {
        cs_set_error("cs_register_revisit_decide_dev: bad arguments");
        return CS_ERR_INVALID;
    }
    RvArgs A;
    memset(&A, 0, sizeof(A));
    if (const int rc = rv_fill("cs_register_revisit_decide_dev", A, nCams, N, P, cap, mapBase, kinds, d_nextLoop, d_visitLoop, d_slot, d_flags, d_mergeable,
                               d_mapFlags, d_pointFeat, d_slot2map, d_attached, d_regOut, d_decideScratch, d_curList, d_curCount, curCap, d_counts,
                               d_overflow))
        return rc;
    A.list = d_list, A.listCount = d_listCount, A.nextList = d_nextList, A.nextCount = d_nextCount;
    CS_HIP(hipSetDevice(device));
    if (nCams <= 8)
        hipLaunchKernelGGL(k_revisit_decide<8>, dim3(1), dim3(cap <= 256 ? 256 : (cap + 63) / 64 * 64), 0, (hipStream_t)hip_stream, A);
    else
        hipLaunchKernelGGL(k_revisit_decide<RD_MAX_CAMS>, dim3(1), dim3(cap <= 256 ? 256 : (cap + 63) / 64 * 64), 0, (hipStream_t)hip_stream, A);
    CS_CHECK_LAUNCH();
    return CS_OK;
}
extern "C" size_t cs_register_decide_scratch_bytes(int nCams, int N, int P) {
    if (nCams < 1 || N < 1 || P < 0) return 0;
    // head | code | base | owner x 3 | active list (at least the RD_MAX_SWEEPS words that stood here before: the size never shrinks) | 4 words
    const size_t nList = (size_t)P > (size_t)RD_MAX_SWEEPS ? (size_t)P : (size_t)RD_MAX_SWEEPS;
    return sizeof(int) * (RD_SCRATCH_HEAD + (size_t)nCams * P + (size_t)P + 3 * (size_t)nCams * N + nList + 4);
}

extern "C" int cs_register_decide_static_dev(int device, void* hip_stream, int nCams, int N, int P, int mapBase, const int* d_slot, const int* d_flags,
                                             const unsigned char* d_mergeable, const unsigned char* d_mapFlags, int* d_pointFeat,
                                             int* const* d_slot2map /* host array of nCams device pointers */, unsigned char* d_attached,
                                             unsigned char* d_regged, void* d_scratch, int nSweeps, int* d_counts) {
    return cs_register_decide_static_cam_dev(device, hip_stream, nCams, N, P, mapBase, d_slot, d_flags, d_mergeable, d_mapFlags, d_pointFeat, d_slot2map,
                                             d_attached, d_regged, d_scratch, nSweeps, d_counts, -1);
}

extern "C" int cs_register_decide_static_cam_dev(int device, void* hip_stream, int nCams, int N, int P, int mapBase, const int* d_slot,
                                                 const int* d_flags, const unsigned char* d_mergeable, const unsigned char* d_mapFlags,
                                                 int* d_pointFeat, int* const* d_slot2map, unsigned char* d_attached, unsigned char* d_regged,
                                                 void* d_scratch, int nSweeps, int* d_counts, int onlyCam) {
    return cs_register_decide_kinds_dev(device, hip_stream, nCams, N, P, mapBase, d_slot, d_flags, d_mergeable, d_mapFlags, d_pointFeat, d_slot2map,
                                        d_attached, d_regged, d_scratch, nSweeps, d_counts, onlyCam, 1);
}

extern "C" int cs_register_decide_kinds_dev(int device, void* hip_stream, int nCams, int N, int P, int mapBase, const int* d_slot, const int* d_flags,
                                            const unsigned char* d_mergeable, const unsigned char* d_mapFlags, int* d_pointFeat,
                                            int* const* d_slot2map, unsigned char* d_attached, unsigned char* d_regged, void* d_scratch,
                                            int nSweeps, int* d_counts, int onlyCam, int kinds) {
    return cs_register_decide_kinds_rounds_dev(device, hip_stream, nCams, N, P, mapBase, d_slot, d_flags, d_mergeable, d_mapFlags, d_pointFeat, d_slot2map,
                                               d_attached, d_regged, d_scratch, nSweeps, d_counts, onlyCam, kinds, nullptr, 0, 0, nullptr, nullptr, nullptr);
}

extern "C" int cs_register_decide_kinds_rounds_dev(int device, void* hip_stream, int nCams, int N, int P, int mapBase, const int* d_slot, const int* d_flags,
                                                   const unsigned char* d_mergeable, const unsigned char* d_mapFlags, int* d_pointFeat,
                                                   int* const* d_slot2map, unsigned char* d_attached, unsigned char* d_regged, void* d_scratch,
                                                   int nSweeps, int* d_counts, int onlyCam, int kinds, int* d_rvLists, int rvCap, int nRounds,
                                                   int* d_rvCounts, int* d_visitLoop, int* d_nextLoop) {
    if (d_rvLists && (rvCap < 1 || rvCap > RV_MAX_ROWS || nRounds < 1 || nRounds > 8 || !d_rvCounts || !d_visitLoop || !d_nextLoop || nSweeps != 0 || onlyCam >= 0)) {
        cs_set_error("cs_register_decide_kinds_rounds_dev: the second visits' lists need 1..%d rows, 1..8 rounds, their counters, visitLoop / nextLoop, "
                     "the self-settling launch (nSweeps 0) and all cameras' loops", RV_MAX_ROWS);
        return CS_ERR_INVALID;
    }
    if (onlyCam >= nCams || kinds < 1 || kinds > 3) {
        cs_set_error("cs_register_decide_kinds_dev: camera %d of %d, kinds %d (1: static, 2: dynamic, 3: both)", onlyCam, nCams, kinds);
        return CS_ERR_INVALID;
    }
    if (nCams < 1 || nCams > RD_MAX_CAMS || N < 1 || P < 0 || (long long)nCams * N > RD_FEAT || (long long)nCams * P * nCams > 0x7fffffffLL ||
        mapBase < 0 || nSweeps < 0 || nSweeps > 256 || !d_slot || !d_flags || !d_mergeable || !d_mapFlags || !d_pointFeat || !d_slot2map ||
        !d_attached || !d_regged || !d_scratch) {
        cs_set_error("cs_register_decide_static_dev: bad arguments (1..%d cameras, 0..256 sweeps)", RD_MAX_CAMS);
        return CS_ERR_INVALID;
    }
    RdArgs A;
    memset(&A, 0, sizeof(A));
    A.nCams = nCams, A.N = N, A.P = P, A.mapBase = mapBase, A.nSweeps = nSweeps, A.onlyCam = onlyCam < 0 ? -1 : onlyCam, A.kinds = kinds;
    A.slot = d_slot, A.flags = d_flags, A.mergeable = d_mergeable, A.mapFlags = d_mapFlags, A.pointFeat = d_pointFeat;
    for (int c = 0; c < nCams; ++c) {
        if (!d_slot2map[c]) {
            cs_set_error("cs_register_decide_static_dev: null slot2map of camera %d", c);
            return CS_ERR_INVALID;
        }
        A.slot2map[c] = d_slot2map[c];
    }
    A.attached = d_attached, A.regged = d_regged, A.counts = d_counts;
    A.rvLists = d_rvLists, A.rvCap = rvCap, A.nRounds = nRounds, A.rvCounts = d_rvCounts, A.visitLoop = d_visitLoop, A.nextLoop = d_nextLoop;
    int* scr = (int*)d_scratch;
    A.ticket = scr, A.nActive = scr + 1, scr += RD_SCRATCH_HEAD;
    A.code = scr, scr += (size_t)nCams * P;
    A.base = scr, scr += P;
    for (int k = 0; k < 3; ++k) A.owner[k] = scr, scr += (size_t)nCams * N;
    A.active = scr, scr += P > RD_MAX_SWEEPS ? P : RD_MAX_SWEEPS;
    A.callFlag = scr + 1, A.timeouts = scr + 2, A.unconverged = scr + 3;
    CS_HIP(hipSetDevice(device));
    if (P == 0) return CS_OK;
    hipStream_t s = (hipStream_t)hip_stream;
    const int ppb = RD_THREADS / nCams, gE = (P + ppb - 1) / ppb, gP = (P + 255) / 256;   // (whole points per workgroup)
    if (nCams <= 8)
        hipLaunchKernelGGL(k_decide_prepare<8>, dim3(gE), dim3(RD_THREADS), 0, s, A);
    else
        hipLaunchKernelGGL(k_decide_prepare<RD_MAX_CAMS>, dim3(gE), dim3(RD_THREADS), 0, s, A);
    if (nSweeps == 0) {   // as many sweeps as the frame needs, in that ONE launch (rd_resolve)
        CS_CHECK_LAUNCH();
        return CS_OK;
    }
    // sweep k reads owner[k % 3], claims into owner[(k + 1) % 3] and clears owner[(k + 2) % 3] for the sweep after it
    for (int k = 0; k < nSweeps; ++k)
        hipLaunchKernelGGL(k_decide_sweep, dim3(gP), dim3(256), 0, s, A, (const int*)A.owner[k % 3], A.owner[(k + 1) % 3], A.owner[(k + 2) % 3],
                           (const int*)nullptr, 0);
    hipLaunchKernelGGL(k_decide_sweep, dim3(gP), dim3(256), 0, s, A, (const int*)A.owner[nSweeps % 3], (int*)nullptr, (int*)nullptr,
                       (const int*)A.owner[(nSweeps + 2) % 3], 1);
    CS_CHECK_LAUNCH();
    return CS_OK;
}

namespace {

// ---- the candidates of a rank's own cameras to every rank (cameras sharded over GPUs) ------------------------------------------------
// pack: columns cam0 .. cam0 + nOwn - 1 of the P x nCams tables slot / flags / mergeable into one send record of 3 * nOwn * P ints
// ([table][own camera][point]); unpack: the gathered records of all ranks (rank r owns cameras r * nOwn ..) back into the tables.
__global__ __launch_bounds__(256) void k_candidates_pack(int P, int nCams, int cam0, int nOwn, const int* __restrict__ slot, const int* __restrict__ flags,
                                                         const unsigned char* __restrict__ merg, int* __restrict__ send) {
    const int q = blockIdx.x * 256 + threadIdx.x;
    if (q >= nOwn * P) return;
    const int i = q / P, p = q - i * P;
    const size_t k = (size_t)p * nCams + cam0 + i;
    send[q] = slot[k], send[nOwn * P + q] = flags[k], send[2 * nOwn * P + q] = merg[k];
}
__global__ __launch_bounds__(256) void k_candidates_unpack(int P, int nCams, int nOwn, int skipRank, const int* __restrict__ recv, int* __restrict__ slot,
                                                           int* __restrict__ flags, unsigned char* __restrict__ merg) {
    const int q = blockIdx.x * 256 + threadIdx.x;
    if (q >= nCams * P) return;
    const int g = q / P, p = q - g * P, r = g / nOwn, i = g - r * nOwn;
    if (r == skipRank) return;
    const int* rec = recv + (size_t)r * 3 * nOwn * P;
    const size_t k = (size_t)p * nCams + g;
    slot[k] = rec[i * P + p], flags[k] = rec[nOwn * P + i * P + p], merg[k] = (unsigned char)rec[2 * nOwn * P + i * P + p];
}

}  // namespace

namespace {
// the same over a LIST of rows (cs_register_list_current_dev: identical on every rank, since every rank holds the same pointFeat table): row j of
// the record = map point list[j], j < cap; entries of rows beyond the list travel as -1 / 0 / 255.  The record stays cap rows long whatever
// the map's capacity is.
__global__ __launch_bounds__(256) void k_candidates_pack_list(int cap, int nCams, int cam0, int nOwn, const int* __restrict__ list,
                                                              const int* __restrict__ slot, const int* __restrict__ flags,
                                                              const unsigned char* __restrict__ merg, int* __restrict__ send) {
    const int q = blockIdx.x * 256 + threadIdx.x;
    if (q >= nOwn * cap) return;
    const int i = q / cap, j = q - i * cap, p = list[j];
    const size_t k = (size_t)(p < 0 ? 0 : p) * nCams + cam0 + i;
    send[q] = p < 0 ? -1 : slot[k], send[nOwn * cap + q] = p < 0 ? 0 : flags[k], send[2 * nOwn * cap + q] = p < 0 ? 255 : merg[k];
}
__global__ __launch_bounds__(256) void k_candidates_unpack_list(int cap, int nCams, int nOwn, int skipRank, const int* __restrict__ list,
                                                                const int* __restrict__ recv, int* __restrict__ slot, int* __restrict__ flags,
                                                                unsigned char* __restrict__ merg) {
    const int q = blockIdx.x * 256 + threadIdx.x;
    if (q >= nCams * cap) return;
    const int g = q / cap, j = q - g * cap, r = g / nOwn, i = g - r * nOwn, p = list[j];
    if (r == skipRank || p < 0) return;
    const int* rec = recv + (size_t)r * 3 * nOwn * cap;
    const size_t k = (size_t)p * nCams + g;
    slot[k] = rec[i * cap + j], flags[k] = rec[nOwn * cap + i * cap + j], merg[k] = (unsigned char)rec[2 * nOwn * cap + i * cap + j];
}
}  // namespace

extern "C" int cs_register_candidates_pack_list_dev(int device, void* hip_stream, int cap, int nCams, int cam0, int nOwn, const int* d_list,
                                                    const int* d_slot, const int* d_flags, const unsigned char* d_mergeable, int* d_send) {
    if (cap < 0 || nCams < 1 || cam0 < 0 || nOwn < 1 || cam0 + nOwn > nCams || !d_list || !d_slot || !d_flags || !d_mergeable || !d_send) {
        cs_set_error("cs_register_candidates_pack_list_dev: bad arguments");
        return CS_ERR_INVALID;
    }
    if (cap == 0) return CS_OK;
    CS_HIP(hipSetDevice(device));
    hipLaunchKernelGGL(k_candidates_pack_list, dim3((nOwn * cap + 255) / 256), dim3(256), 0, (hipStream_t)hip_stream, cap, nCams, cam0, nOwn, d_list,
                       d_slot, d_flags, d_mergeable, d_send);
    CS_CHECK_LAUNCH();
    return CS_OK;
}
extern "C" int cs_register_candidates_unpack_list_dev(int device, void* hip_stream, int cap, int nCams, int nOwn, int skipRank, const int* d_list,
                                                      const int* d_recv, int* d_slot, int* d_flags, unsigned char* d_mergeable) {
    if (cap < 0 || nCams < 1 || nOwn < 1 || nCams % nOwn || !d_list || !d_recv || !d_slot || !d_flags || !d_mergeable) {
        cs_set_error("cs_register_candidates_unpack_list_dev: bad arguments");
        return CS_ERR_INVALID;
    }
    if (cap == 0) return CS_OK;
    CS_HIP(hipSetDevice(device));
    hipLaunchKernelGGL(k_candidates_unpack_list, dim3((nCams * cap + 255) / 256), dim3(256), 0, (hipStream_t)hip_stream, cap, nCams, nOwn, skipRank,
                       d_list, d_recv, d_slot, d_flags, d_mergeable);
    CS_CHECK_LAUNCH();
    return CS_OK;
}

extern "C" int cs_register_candidates_pack_dev(int device, void* hip_stream, int P, int nCams, int cam0, int nOwn, const int* d_slot,
                                               const int* d_flags, const unsigned char* d_mergeable, int* d_send) {
    if (P < 1 || nCams < 1 || cam0 < 0 || nOwn < 1 || cam0 + nOwn > nCams || !d_slot || !d_flags || !d_mergeable || !d_send) {
        cs_set_error("cs_register_candidates_pack_dev: bad arguments");
        return CS_ERR_INVALID;
    }
    CS_HIP(hipSetDevice(device));
    hipLaunchKernelGGL(k_candidates_pack, dim3((nOwn * P + 255) / 256), dim3(256), 0, (hipStream_t)hip_stream, P, nCams, cam0, nOwn, d_slot, d_flags,
                       d_mergeable, d_send);
    CS_CHECK_LAUNCH();
    return CS_OK;
}
extern "C" int cs_register_candidates_unpack_dev(int device, void* hip_stream, int P, int nCams, int nOwn, int skipRank, const int* d_recv, int* d_slot,
                                                 int* d_flags, unsigned char* d_mergeable) {
    if (P < 1 || nCams < 1 || nOwn < 1 || nCams % nOwn || !d_recv || !d_slot || !d_flags || !d_mergeable) {
        cs_set_error("cs_register_candidates_unpack_dev: bad arguments");
        return CS_ERR_INVALID;
    }
    CS_HIP(hipSetDevice(device));
    hipLaunchKernelGGL(k_candidates_unpack, dim3((nCams * P + 255) / 256), dim3(256), 0, (hipStream_t)hip_stream, P, nCams, nOwn, skipRank, d_recv,
                       d_slot, d_flags, d_mergeable);
    CS_CHECK_LAUNCH();
    return CS_OK;
}

namespace {
}  // namespace

// Host-pointer form for the reference's loops: one upload, one launch, one read-back.  cams[c] holds HOST pointers.
extern "C" int cs_register_search(int device, int nCams, const cs_register_cam* cams, int N, int W, int H, int P, const double* M,
                                  const double* cov, const int* pointFeat, double sigmaSearch, double maxDist, double sigmaMerge,
                                  int* slot, double* m, double* var, double* dist, int* flags) {
    int rc = check_args("cs_register_search", nCams, cams, N, W, H, P, sigmaSearch, maxDist, sigmaMerge);
    if (rc != CS_OK) return rc;
    if (P == 0) return CS_OK;
    if (!M || !cov || !pointFeat || !slot || !m || !var || !dist || !flags) {
        cs_set_error("cs_register_search: null pointer");
        return CS_ERR_INVALID;
    }
    CS_HIP(hipSetDevice(device));
    const size_t pairs = (size_t)P * nCams;
    // one staging block: per camera K R t | xy | state | slot2map | isDynamic, then M | cov | pointFeat, then the outputs
    const size_t camBytes = (21 + 2 * (size_t)N) * 8 + 2 * (size_t)N * 4 + (((size_t)N + 7) & ~(size_t)7);
    const size_t inBytes = camBytes * nCams + (size_t)P * 12 * 8 + ((pairs * 4 + 7) & ~(size_t)7);
    const size_t outBytes = pairs * (2 + 4 + 1) * 8 + 2 * ((pairs * 4 + 7) & ~(size_t)7);
    char *h = nullptr, *d = nullptr;
    CS_HIP(hipHostMalloc((void**)&h, inBytes + outBytes, hipHostMallocDefault));
    if (hipMalloc((void**)&d, inBytes + outBytes) != hipSuccess) {
        (void)hipHostFree(h);
        cs_set_error("cs_register_search: out of device memory");
        return CS_ERR_HIP;
    }
    cs_register_cam dc[RG_MAX_CAMS];
    size_t off = 0;
    for (int c = 0; c < nCams; ++c) {
        const cs_register_cam& q = cams[c];
        if (!q.K || !q.R || !q.t || !q.xy || !q.state || !q.slot2map) {
            (void)hipHostFree(h);
            (void)hipFree(d);
            cs_set_error("cs_register_search: null pointer in camera %d", c);
            return CS_ERR_INVALID;
        }
        memcpy(h + off, q.K, 72);
        dc[c].K = (const double*)(d + off);
        memcpy(h + off + 72, q.R, 72);
        dc[c].R = (const double*)(d + off + 72);
        memcpy(h + off + 144, q.t, 24);
        dc[c].t = (const double*)(d + off + 144);
        size_t o2 = off + 168;
        memcpy(h + o2, q.xy, 2 * (size_t)N * 8);
        dc[c].xy = (const double*)(d + o2);
        o2 += 2 * (size_t)N * 8;
        memcpy(h + o2, q.state, (size_t)N * 4);
        dc[c].state = (const int*)(d + o2);
        o2 += (size_t)N * 4;
        memcpy(h + o2, q.slot2map, (size_t)N * 4);
        dc[c].slot2map = (const int*)(d + o2);
        o2 += (size_t)N * 4;
        dc[c].isStatic = nullptr;
        if (q.isDynamic) {
            memcpy(h + o2, q.isDynamic, (size_t)N);
            dc[c].isDynamic = (const unsigned char*)(d + o2);
        } else if (q.isStatic) {   // (staged as its complement)
            for (int i = 0; i < N; ++i) h[o2 + i] = q.isStatic[i] ? 0 : 1;
            dc[c].isDynamic = (const unsigned char*)(d + o2);
        } else {
            dc[c].isDynamic = nullptr;
        }
        off += camBytes;
    }
    const size_t oM = off, oC = oM + (size_t)P * 24, oF = oC + (size_t)P * 72;
    memcpy(h + oM, M, (size_t)P * 24);
    memcpy(h + oC, cov, (size_t)P * 72);
    memcpy(h + oF, pointFeat, pairs * 4);
    const size_t pad4 = (pairs * 4 + 7) & ~(size_t)7;
    const size_t om = inBytes, ov = om + pairs * 16, od = ov + pairs * 32, os = od + pairs * 8, ofl = os + pad4;
    hipStream_t s = nullptr;
    hipError_t e = hipMemcpyAsync(d, h, inBytes, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) {
        rc = cs_register_search_dev(device, s, nCams, dc, N, W, H, P, (const double*)(d + oM), (const double*)(d + oC),
                                    (const int*)(d + oF), sigmaSearch, maxDist, sigmaMerge, (int*)(d + os), (double*)(d + om),
                                    (double*)(d + ov), (double*)(d + od), (int*)(d + ofl));
        if (rc == CS_OK) e = hipMemcpyAsync(h + inBytes, d + inBytes, outBytes, hipMemcpyDeviceToHost, s);
        if (rc == CS_OK && e == hipSuccess) e = hipStreamSynchronize(s);
    }
    if (rc == CS_OK && e == hipSuccess) {
        memcpy(m, h + om, pairs * 16);
        memcpy(var, h + ov, pairs * 32);
        memcpy(dist, h + od, pairs * 8);
        memcpy(slot, h + os, pairs * 4);
        memcpy(flags, h + ofl, pairs * 4);
    }
    (void)hipHostFree(h);
    (void)hipFree(d);
    if (rc != CS_OK) return rc;
    if (e != hipSuccess) {
        cs_set_error("cs_register_search: %s", hipGetErrorString(e));
        return CS_ERR_HIP;
    }
    return CS_OK;
}
