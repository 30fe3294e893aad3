// export.hip -- a frame loop's result files from its device state (cs_loop_export_results): what CoSLAM::exportResults delivers at the
// end of a run (reference src/gui/CoSLAMThread.cpp, behind the frame loop; src/app/SL_CoSLAM.cpp:1914-2028), assembled on the device
// from the pose history (store + whole-run archive: cs_track_history_set_archive), the feature references (cs_feat_ref [nMap][nCams])
// with the history's linked-segment pools, and the map -- then written by the host writer of results.cpp (cs_export_results_v1).
//
// Once per run, so the kernels are plain:
//   k_exp_count      one lane per (map point, camera): the point's chain in the camera -- the run [first, frame] of its reference, then
//                    every linked segment [first, last] -- walked WITHOUT the per-frame walks' node bound; per node (camera, frame) a
//                    count; a point with at least one node is marked (getAllStaticMapPoints lists only points some feature carries)
//   k_exp_scan       one workgroup: exclusive prefix sums (the per-(camera, frame) counts -> featPtr; the marks -> the static list)
//   k_exp_fill       the same walks again: every node's key (slot << 32 | point) into its (camera, frame) row, in any order
//   k_exp_sort_fill  one workgroup per (camera, frame) row: bitonic sort of the keys in LDS -- slot order, which is the order of
//                    m_featPts.getFrame, ties by map index -- then the point ids and the frame's pixels of the slots
//   k_exp_points     the static list: ids (= map indices), positions, covariances, compacted in ascending map index
//   k_exp_poses      every camera's pose of every frame from the history's first frame: archive, then store
// Only the finished arrays are copied to the host.
#include <vector>

#include "cs_common.h"
#include "history_view.h"

namespace {

constexpr int EXP_SORT_MAX = 4096;   // features of one (camera, frame) row the sort holds in LDS (32 KB); a row holds at most N without
                                     // two points sharing a feature

struct ExpArgs {
    CsHistView v;
    int F0, nF, nMap;
    const int4* ref;              // [nMap][nCams]
    const unsigned char* flags;   // [nMap]
};

__device__ __forceinline__ bool exp_certain_static(unsigned char f) { return (f & (CS_MAP_DYNAMIC | CS_MAP_FALSE | CS_MAP_UNCERTAIN)) == 0; }

// the entry of frame f of camera c: archive or store
__device__ __forceinline__ size_t exp_entry(const CsHistView& v, int c, int f, bool& arch) {
    arch = v.archCount > 0 && f < v.archFirst + v.archCount;
    if (arch) return (size_t)c * v.archCap + (f - v.archFirst);
    return (size_t)c * v.H + ((v.head - (v.lastFrame - f)) % v.H + v.H) % v.H;
}

// every node (slot, frame) of the chain behind reference r in camera c, frames F0 .. lastFrame; no bound on the number of nodes (the pool
// is finite: a chain that came back to a segment it passed would be walked at most nSeg times round)
template <class Fn>
__device__ void exp_walk(const ExpArgs& A, int c, int4 r, Fn&& fn) {
    if (r.x < 0) return;
    const int nSeg = min(A.v.segCount[c], A.v.segCap);
    int slot = r.x, hi = r.y, lo = r.z, seg = r.w;
    for (int hop = 0;; ++hop) {
        if (slot >= 0 && slot < A.v.N) {
            const int a = max(lo, A.F0), b = min(hi, A.v.lastFrame);
            for (int f = a; f <= b; ++f) fn(slot, f);
        }
        if (seg < 0 || seg >= nSeg || hop >= nSeg) break;
        const int4 g = A.v.segPool[(size_t)c * A.v.segCap + seg];
        slot = g.x, hi = g.y, lo = g.z, seg = g.w;
    }
}

__global__ __launch_bounds__(256) void k_exp_count(ExpArgs A, int* cnt, int* has, unsigned long long* stats) {
    const int q = blockIdx.x * 256 + threadIdx.x, nC = A.v.nCams;
    if (q >= A.nMap * nC) return;
    const int p = q / nC, c = q - p * nC;
    if (!exp_certain_static(A.flags[p])) return;
    unsigned long long n = 0, nArch = 0;
    const int archEnd = A.v.archCount > 0 ? A.v.archFirst + A.v.archCount : A.F0;
    exp_walk(A, c, A.ref[q], [&](int, int f) {
        atomicAdd(cnt + (size_t)c * A.nF + (f - A.F0), 1);
        ++n;
        nArch += f < archEnd;
    });
    if (n) {
        has[p] = 1;
        atomicAdd(stats + 1, n);
        atomicAdd(stats + 2, nArch);
    }
}

// exclusive prefix sums of in[0 .. n) into out[0 .. n], out[n] = the total; one workgroup of 1024 lanes, a contiguous chunk each
__global__ __launch_bounds__(1024) void k_exp_scan(const int* __restrict__ in, int* __restrict__ out, int n) {
    __shared__ int part[1024];
    const int t = threadIdx.x, per = (n + 1023) / 1024, a = min(t * per, n), b = min(a + per, n);
    int s = 0;
    for (int i = a; i < b; ++i) s += in[i];
    part[t] = s;
    __syncthreads();
    for (int off = 1; off < 1024; off <<= 1) {
        const int v = t >= off ? part[t - off] : 0;
        __syncthreads();
        part[t] += v;
        __syncthreads();
    }
    int run = part[t] - s;
    for (int i = a; i < b; ++i) {
        out[i] = run;
        run += in[i];
    }
    if (t == 1023) out[n] = part[1023];
}

__global__ __launch_bounds__(256) void k_exp_fill(ExpArgs A, const int* __restrict__ ptr, int* cur, unsigned long long* keys) {
    const int q = blockIdx.x * 256 + threadIdx.x, nC = A.v.nCams;
    if (q >= A.nMap * nC) return;
    const int p = q / nC, c = q - p * nC;
    if (!exp_certain_static(A.flags[p])) return;
    exp_walk(A, c, A.ref[q], [&](int slot, int f) {
        const size_t row = (size_t)c * A.nF + (f - A.F0);
        const int k = ptr[row] + atomicAdd(cur + row, 1);
        keys[k] = ((unsigned long long)slot << 32) | (unsigned)p;
    });
}

__global__ __launch_bounds__(256) void k_exp_sort_fill(ExpArgs A, const int* __restrict__ ptr, const unsigned long long* __restrict__ keys,
                                                       long long* outId, double* outXY, int* err) {
    __shared__ unsigned long long s[EXP_SORT_MAX];
    const int row = blockIdx.x, c = row / A.nF, f = A.F0 + (row - c * A.nF);
    const int base = ptr[row], n = ptr[row + 1] - base;
    if (n == 0) return;
    if (n > EXP_SORT_MAX) {
        if (threadIdx.x == 0) atomicMax(err, n);
        return;
    }
    int P = 1;
    while (P < n) P <<= 1;
    for (int i = threadIdx.x; i < P; i += 256) s[i] = i < n ? keys[base + i] : ~0ull;
    __syncthreads();
    for (int k = 2; k <= P; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = threadIdx.x; i < P; i += 256) {
                const int l = i ^ j;
                if (l > i) {
                    const unsigned long long a = s[i], b = s[l];
                    if ((a > b) == ((i & k) == 0)) s[i] = b, s[l] = a;
                }
            }
            __syncthreads();
        }
    bool arch;
    const size_t e = exp_entry(A.v, c, f, arch);
    const double* xy = (arch ? A.v.archXY : A.v.xy) + e * 2 * A.v.N;
    for (int i = threadIdx.x; i < n; i += 256) {
        const unsigned long long key = s[i];
        const int slot = (int)(key >> 32), p = (int)(key & 0xffffffffu);
        outId[base + i] = p;
        outXY[2 * (size_t)(base + i)] = xy[slot];
        outXY[2 * (size_t)(base + i) + 1] = xy[A.v.N + slot];
    }
}

__global__ __launch_bounds__(256) void k_exp_points(int nMap, const int* __restrict__ has, const int* __restrict__ pos, const double* __restrict__ M,
                                                    const double* __restrict__ cov, long long* outId, double* outM, double* outCov) {
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= nMap || !has[p]) return;
    const int k = pos[p];
    outId[k] = p;
    for (int e = 0; e < 3; ++e) outM[3 * (size_t)k + e] = M[3 * (size_t)p + e];
    for (int e = 0; e < 9; ++e) outCov[9 * (size_t)k + e] = cov[9 * (size_t)p + e];
}

// camera-major [nCams][nF][9] / [3]
__global__ __launch_bounds__(256) void k_exp_poses(CsHistView v, int F0, int nF, double* R, double* t) {
    const size_t q = (size_t)blockIdx.x * 256 + threadIdx.x, i = q / 12;
    const int e = (int)(q - 12 * i);
    if (i >= (size_t)v.nCams * nF) return;
    const int c = (int)(i / nF), f = F0 + (int)(i - (size_t)c * nF);
    bool arch;
    const size_t en = exp_entry(v, c, f, arch);
    if (e < 9)
        R[9 * i + e] = (arch ? v.archR : v.R)[en * 9 + e];
    else
        t[3 * i + (e - 9)] = (arch ? v.archT : v.t)[en * 3 + (e - 9)];
}

// device scratch of one export, freed on every way out
struct ExpBufs {
    std::vector<void*> p;
    template <class T>
    int get(T** out, size_t n) {
        *out = nullptr;
        if (hipMalloc((void**)out, sizeof(T) * (n ? n : 1)) != hipSuccess) {
            cs_set_error("cs_loop_export_results: hipMalloc of %zu bytes failed", sizeof(T) * n);
            return CS_ERR_HIP;
        }
        p.push_back(*out);
        return CS_OK;
    }
    ~ExpBufs() {
        for (void* q : p) (void)hipFree(q);
    }
};

}  // namespace

extern "C" int cs_loop_export_results(const char* dirPath, const cs_track_history* h, void* hip_stream, const cs_feat_ref* d_featRef, int nMap,
                                      const double* d_M, const double* d_cov, const unsigned char* d_mapFlags, const cs_loop_export_cam* cams,
                                      int covAsReference, long long* stats) {
    if (!dirPath || !h || !d_featRef || nMap < 1 || !d_M || !d_cov || !d_mapFlags || !cams) {
        cs_set_error("cs_loop_export_results: bad arguments");
        return CS_ERR_INVALID;
    }
    ExpArgs A;
    memset(&A, 0, sizeof(A));
    cs_history_view(h, &A.v);
    const CsHistView& v = A.v;
    for (int c = 0; c < v.nCams; ++c)
        if (!cams[c].videoFilePath || !cams[c].K || !cams[c].kc) {
            cs_set_error("cs_loop_export_results: camera %d: null video path, K or kc", c);
            return CS_ERR_INVALID;
        }
    if (v.stored < 1) {
        cs_set_error("cs_loop_export_results: the history holds no frame");
        return CS_ERR_INVALID;
    }
    A.F0 = v.archCount > 0 ? v.archFirst : v.lastFrame - v.stored + 1;
    if (A.F0 > v.firstFrame) {
        cs_set_error("cs_loop_export_results: frames %d..%d have left the store and no archive holds them (cs_track_history_set_archive)",
                     v.firstFrame, A.F0 - 1);
        return CS_ERR_INVALID;
    }
    A.nF = v.lastFrame - A.F0 + 1, A.nMap = nMap;
    A.ref = (const int4*)d_featRef, A.flags = d_mapFlags;
    const int nC = v.nCams, rows = nC * A.nF;
    CS_HIP(hipSetDevice(v.device));
    hipStream_t s = (hipStream_t)hip_stream;
    ExpBufs B;
    int *cnt, *cur, *ptr, *has, *pos, *err;
    unsigned long long* dStats;
    double *pR, *pT;
    int rc;
    if ((rc = B.get(&cnt, rows)) || (rc = B.get(&cur, rows)) || (rc = B.get(&ptr, rows + 1)) || (rc = B.get(&has, nMap)) ||
        (rc = B.get(&pos, nMap + 1)) || (rc = B.get(&err, 1)) || (rc = B.get(&dStats, 3)) || (rc = B.get(&pR, 9 * (size_t)rows)) ||
        (rc = B.get(&pT, 3 * (size_t)rows)))
        return rc;
    CS_HIP(hipMemsetAsync(cnt, 0, sizeof(int) * rows, s));
    CS_HIP(hipMemsetAsync(cur, 0, sizeof(int) * rows, s));
    CS_HIP(hipMemsetAsync(has, 0, sizeof(int) * nMap, s));
    CS_HIP(hipMemsetAsync(err, 0, sizeof(int), s));
    CS_HIP(hipMemsetAsync(dStats, 0, 3 * sizeof(unsigned long long), s));
    const unsigned lanes = (unsigned)(((size_t)nMap * nC + 255) / 256);
    hipLaunchKernelGGL(k_exp_count, dim3(lanes), dim3(256), 0, s, A, cnt, has, dStats);
    hipLaunchKernelGGL(k_exp_scan, dim3(1), dim3(1024), 0, s, (const int*)cnt, ptr, rows);
    hipLaunchKernelGGL(k_exp_scan, dim3(1), dim3(1024), 0, s, (const int*)has, pos, nMap);
    hipLaunchKernelGGL(k_exp_poses, dim3((unsigned)((12 * (size_t)rows + 255) / 256)), dim3(256), 0, s, v, A.F0, A.nF, pR, pT);
    CS_CHECK_LAUNCH();
    int nFeat = 0, nPts = 0;
    CS_HIP(hipMemcpyAsync(&nFeat, ptr + rows, sizeof(int), hipMemcpyDeviceToHost, s));
    CS_HIP(hipMemcpyAsync(&nPts, pos + nMap, sizeof(int), hipMemcpyDeviceToHost, s));
    CS_HIP(hipStreamSynchronize(s));
    unsigned long long* keys;
    long long *fId, *ptId;
    double *fXY, *ptM, *ptCov;
    if ((rc = B.get(&keys, nFeat)) || (rc = B.get(&fId, nFeat)) || (rc = B.get(&fXY, 2 * (size_t)nFeat)) || (rc = B.get(&ptId, nPts)) ||
        (rc = B.get(&ptM, 3 * (size_t)nPts)) || (rc = B.get(&ptCov, 9 * (size_t)nPts)))
        return rc;
    hipLaunchKernelGGL(k_exp_fill, dim3(lanes), dim3(256), 0, s, A, (const int*)ptr, cur, keys);
    hipLaunchKernelGGL(k_exp_sort_fill, dim3(rows), dim3(256), 0, s, A, (const int*)ptr, (const unsigned long long*)keys, fId, fXY, err);
    hipLaunchKernelGGL(k_exp_points, dim3((nMap + 255) / 256), dim3(256), 0, s, nMap, (const int*)has, (const int*)pos, d_M, d_cov, ptId, ptM, ptCov);
    CS_CHECK_LAUNCH();
    std::vector<int> hPtr(rows + 1);
    std::vector<long long> hId(nFeat), hPtId(nPts);
    std::vector<double> hXY(2 * (size_t)nFeat), hM(3 * (size_t)nPts), hCov(9 * (size_t)nPts), hR(9 * (size_t)rows), hT(3 * (size_t)rows);
    int hErr = 0;
    unsigned long long hStats[3] = {0, 0, 0};
    CS_HIP(hipMemcpyAsync(hPtr.data(), ptr, sizeof(int) * (rows + 1), hipMemcpyDeviceToHost, s));
    CS_HIP(hipMemcpyAsync(hId.data(), fId, sizeof(long long) * nFeat, hipMemcpyDeviceToHost, s));
    CS_HIP(hipMemcpyAsync(hXY.data(), fXY, sizeof(double) * 2 * nFeat, hipMemcpyDeviceToHost, s));
    CS_HIP(hipMemcpyAsync(hPtId.data(), ptId, sizeof(long long) * nPts, hipMemcpyDeviceToHost, s));
    CS_HIP(hipMemcpyAsync(hM.data(), ptM, sizeof(double) * 3 * nPts, hipMemcpyDeviceToHost, s));
    CS_HIP(hipMemcpyAsync(hCov.data(), ptCov, sizeof(double) * 9 * nPts, hipMemcpyDeviceToHost, s));
    CS_HIP(hipMemcpyAsync(hR.data(), pR, sizeof(double) * 9 * rows, hipMemcpyDeviceToHost, s));
    CS_HIP(hipMemcpyAsync(hT.data(), pT, sizeof(double) * 3 * rows, hipMemcpyDeviceToHost, s));
    CS_HIP(hipMemcpyAsync(&hErr, err, sizeof(int), hipMemcpyDeviceToHost, s));
    CS_HIP(hipMemcpyAsync(hStats, dStats, sizeof(hStats), hipMemcpyDeviceToHost, s));
    CS_HIP(hipStreamSynchronize(s));
    if (hErr) {
        cs_set_error("cs_loop_export_results: a (camera, frame) row carries %d features, more than the %d the sort holds", hErr, EXP_SORT_MAX);
        return CS_ERR_INVALID;
    }
    if (stats) stats[0] = nPts, stats[1] = (long long)hStats[1], stats[2] = (long long)hStats[2];
    std::vector<int> poseFrame(A.nF), featPtr((size_t)nC * (A.nF + 1));
    for (int r = 0; r < A.nF; ++r) poseFrame[r] = A.F0 + r;
    std::vector<cs_export_cam> ec(nC);
    for (int c = 0; c < nC; ++c) {
        const int b0 = hPtr[(size_t)c * A.nF];
        int* fp = featPtr.data() + (size_t)c * (A.nF + 1);
        for (int r = 0; r <= A.nF; ++r) fp[r] = hPtr[(size_t)c * A.nF + r] - b0;
        cs_export_cam& q = ec[c];
        q.videoFilePath = cams[c].videoFilePath, q.K = cams[c].K, q.kc = cams[c].kc, q.W = cams[c].W, q.H = cams[c].H;
        q.startFrameInVideo = cams[c].startFrameInVideo;
        q.nPoses = A.nF, q.poseFrame = poseFrame.data();
        q.poseR = hR.data() + 9 * (size_t)c * A.nF, q.poseT = hT.data() + 3 * (size_t)c * A.nF;
        q.featPtr = fp, q.featPointId = hId.data() + b0, q.featXY = hXY.data() + 2 * (size_t)b0;
    }
    return cs_export_results_v1(dirPath, nC, ec.data(), v.lastFrame, nPts, hPtId.data(), hM.data(), hCov.data(), covAsReference);
}
