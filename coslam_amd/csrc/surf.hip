// surf.hip -- SURF key points and descriptors on the device: ::detectSURFPoints of mergeCamGroups (reference
// src/app/SL_MergeCameraGroup.cpp:308-313).  The reference's SURF is external; the definition is this project's, restated in numpy by
// tests/surf_ref.py.  All cameras of a call in each launch, one stream, no host wait.  Exact layers first (integer box sums, f64 responses
// in one expression order, orders from ballots and scans); only atan2 / cos / sin may differ from the restatement by ulps.
// EVERY integral read goes through sf_box, which clamps its corners into the image.
#include <cmath>

#include "cs_common.h"
#include "dev_arena.h"

namespace {

constexpr int SF_T = 256;                 // threads of a workgroup: 4 waves
constexpr int SF_MAX_CAMS = 16, SF_MAX_PTS = 32768;
constexpr int SF_NL = CS_SURF_MAX_OCTAVES * CS_SURF_MAX_LAYERS;
constexpr int SF_MAX_GROUPS = CS_SURF_MAX_OCTAVES * 4;   // (octave, middle layer)
constexpr int SF_ORI = CS_SURF_ORI_SAMPLES, SF_WIN = CS_SURF_ORI_WINDOWS;
constexpr double SF_TWO_PI = 2.0 * 3.141592653589793;
constexpr double SF_WIN_STEP = 3.141592653589793 / 36.0, SF_WIN_WIDTH = 3.141592653589793 / 3.0;
typedef unsigned long long sf_u64;
constexpr int SF_SEL_PASSES = 8;          // a 64-bit key, 8 bits a pass, from the top
struct SfSel {
    sf_u64 prefix;   // the cut's digits so far, in place
    int need;        // keys to keep among those that share the prefix; <= 0: the camera keeps everything (total <= maxPts)
    int bin;         // keys in the digit the last pass chose
};

struct SurfArgs {
    const unsigned char* img[SF_MAX_CAMS];
    int pitch;
    unsigned* integral;
    double* det;
    unsigned char* lap;
    unsigned char* flag;      // [nCams][nFlat]: the sample is a key point
    int* blockCnt;            // [nCams][nBlocks]
    int* blockOff;            // [nCams][nBlocks]: key points in front of the block
    double* pts;
    float* desc;
    double *size, *angle, *response;
    unsigned char* laplacian;
    int *octave, *layer, *cell, *count, *overflow;
    const double *oriW, *oriGrid /* [109][2] */, *descW;
    int W, H, maxPts, nOct, nLay, dim, mapElems, nFlat, nBlocks, nGroups;
    int mapW[CS_SURF_MAX_OCTAVES], mapH[CS_SURF_MAX_OCTAVES], mapOff[SF_NL], layerSize[SF_NL], layerFits[SF_NL];
    int grpStart[SF_MAX_GROUPS + 1], grpO[SF_MAX_GROUPS], grpM[SF_MAX_GROUPS], grpMargin[SF_MAX_GROUPS];
    double thr;
    // the strongest-first choice (CS_SURF_KEEP_STRONGEST); dropped is null in CS_SURF_KEEP_FIRST and nothing below is touched then
    unsigned* selHist;        // [nCams][SF_SEL_PASSES][256]: digit counts of the candidates' keys, zeroed by the call
    struct SfSel* selState;   // [nCams][SF_SEL_PASSES + 1]: the select in front of pass p (entry 0 is never stored: {0, maxPts})
    int* nWork;               // [nCams]: blocks that hold a candidate, zeroed by the call
    int* tieCnt;              // [nCams][nBlocks]: candidates AT the cut per block, zeroed by the call (selHist, nWork and this are one range)
    int* tieOff;              // [nCams][nBlocks]: ... and in front of the block
    int* workList;            // [nCams][nBlocks]: those blocks, in no order
    int* dropped;             // [nCams]: total - maxPts where the select ran, else 0
};

__device__ __forceinline__ const unsigned* sf_integral(const SurfArgs& A, int c) {
    return A.integral + (size_t)c * (size_t)(A.H + 1) * (size_t)(A.W + 1);
}

// the sum over rows [r0, r1) and columns [c0, c1) with every corner clamped into [0, H] x [0, W]
__device__ __forceinline__ long long sf_box(const unsigned* I, int W, int H, int r0, int c0, int r1, int c1) {
    r0 = cs_clampi(r0, 0, H), r1 = cs_clampi(r1, 0, H), c0 = cs_clampi(c0, 0, W), c1 = cs_clampi(c1, 0, W);
    const int S = W + 1;
    return (long long)I[r1 * S + c1] - (long long)I[r0 * S + c1] - (long long)I[r1 * S + c0] + (long long)I[r0 * S + c0];
}

// (right half - left half, lower half - upper half) of the h x h box with top-left (r - h/2, c - h/2), split at (r, c)
__device__ __forceinline__ void sf_haar(const unsigned* I, int W, int H, int r, int c, int h, long long& hx, long long& hy) {
    const int r0 = r - h / 2, c0 = c - h / 2, r1 = r0 + h, c1 = c0 + h;
    hx = sf_box(I, W, H, r0, c, r1, c1) - sf_box(I, W, H, r0, c0, r1, c);
    hy = sf_box(I, W, H, r, c0, r1, c1) - sf_box(I, W, H, r0, c0, r, c1);
}

// a double to the nearest pixel, floor(v + 0.5), held to a range every later sum stays an int in (the boxes clamp anyway)
__device__ __forceinline__ int sf_round(double v) {
    const double f = floor(v + 0.5);
    return f > -1.0e6 ? (f < 1.0e6 ? (int)f : 1000000) : -1000000;   // (a NaN goes to -1e6)
}

// ---- integral image: a wave per row (prefix sums over chunks of 64), then a thread per column ---------------------------------------
__global__ __launch_bounds__(64) void k_surf_rows(SurfArgs A) {
    const int c = blockIdx.y, y = blockIdx.x, lane = threadIdx.x;
    const unsigned char* img = A.img[c];
    if (!img) return;
    unsigned* row = const_cast<unsigned*>(sf_integral(A, c)) + (size_t)(y + 1) * (A.W + 1);
    if (lane == 0) row[0] = 0;
    unsigned carry = 0;
    for (int x0 = 0; x0 < A.W; x0 += 64) {
        const int x = x0 + lane;
        unsigned v = x < A.W ? img[(size_t)y * A.pitch + x] : 0u;
        for (int d = 1; d < 64; d <<= 1) {
            const unsigned o = __shfl_up(v, d, 64);
            if (lane >= d) v += o;
        }
        if (x < A.W) row[x + 1] = carry + v;
        carry += __shfl(v, 63, 64);
    }
}

__global__ __launch_bounds__(SF_T) void k_surf_cols(SurfArgs A) {
    const int c = blockIdx.y, x = blockIdx.x * SF_T + threadIdx.x;
    if (!A.img[c] || x > A.W) return;
    unsigned* I = const_cast<unsigned*>(sf_integral(A, c));
    const int S = A.W + 1;
    I[x] = 0;
    unsigned acc = 0;
    for (int y = 1; y <= A.H; ++y) {
        acc += I[(size_t)y * S + x];
        I[(size_t)y * S + x] = acc;
    }
}

// ---- fast-Hessian layers: every (camera, octave, layer, sample) in one grid -----------------------------------------------------------
__global__ __launch_bounds__(SF_T) void k_surf_response(SurfArgs A) {
    const int c = blockIdx.z, ol = blockIdx.y, o = ol / CS_SURF_MAX_LAYERS;
    if (!A.img[c] || A.mapOff[ol] < 0 || !A.layerFits[ol]) return;
    const int mw = A.mapW[o], mh = A.mapH[o], e = blockIdx.x * SF_T + threadIdx.x;
    if (e >= mw * mh) return;
    const int i = e / mw, j = e - i * mw, r = i << o, cc = j << o;
    const int L = A.layerSize[ol], lb = L / 3, b = L / 2, W = A.W, H = A.H;
    const unsigned* I = sf_integral(A, c);
    // the L x L window with top-left (r - L/2, c - L/2), cut into 3 x 3 squares of lb: Dxx the middle row of squares (the middle one -2),
    // Dyy the middle column, Dxy the four lb x lb squares about the window's centre (a gap of one pixel when L is odd)
    const int r0 = r - b, c0 = cc - b, q = L - b;
    const long long mid = 3 * sf_box(I, W, H, r0 + lb, c0 + lb, r0 + 2 * lb, c0 + 2 * lb);
    const long long Dxx = sf_box(I, W, H, r0 + lb, c0, r0 + 2 * lb, c0 + L) - mid;
    const long long Dyy = sf_box(I, W, H, r0, c0 + lb, r0 + L, c0 + 2 * lb) - mid;
    const long long Dxy = sf_box(I, W, H, r0 + b - lb, c0 + b - lb, r0 + b, c0 + b) + sf_box(I, W, H, r0 + q, c0 + q, r0 + q + lb, c0 + q + lb) -
                          sf_box(I, W, H, r0 + b - lb, c0 + q, r0 + b, c0 + q + lb) - sf_box(I, W, H, r0 + q, c0 + b - lb, r0 + q + lb, c0 + b);
    const double area = (double)((long long)L * L);
    const double dx = (double)Dxx / area, dy = (double)Dyy / area, dxy = (double)Dxy / area;
    const size_t at = (size_t)c * A.mapElems + A.mapOff[ol] + e;
    A.det[at] = (dx * dy) - ((0.81 * dxy) * dxy);
    A.lap[at] = (dx + dy) > 0.0 ? 1 : 0;
}

// ---- maxima ----------------------------------------------------------------------------------------------------------------------------
struct SfKey {
    double x, y, size, response;
};

// the 3 x 3 Newton step about sample (i, j) of the middle layer N1: an explicit adjugate solve, the expressions of tests/surf_ref.py
__device__ bool sf_newton(const double* N0, const double* N1, const double* N2, int mw, int i, int j, int o, int L, SfKey& K) {
    const int p = i * mw + j;
    const double v = N1[p];
    const double g0 = (N1[p + 1] - N1[p - 1]) * 0.5, g1 = (N1[p + mw] - N1[p - mw]) * 0.5, g2 = (N2[p] - N0[p]) * 0.5;
    const double a = (N1[p + 1] + N1[p - 1]) - 2.0 * v, d = (N1[p + mw] + N1[p - mw]) - 2.0 * v, f = (N2[p] + N0[p]) - 2.0 * v;
    const double b = ((N1[p + mw + 1] - N1[p + mw - 1]) - (N1[p - mw + 1] - N1[p - mw - 1])) * 0.25;
    const double cc = ((N2[p + 1] - N2[p - 1]) - (N0[p + 1] - N0[p - 1])) * 0.25;
    const double e = ((N2[p + mw] - N2[p - mw]) - (N0[p + mw] - N0[p - mw])) * 0.25;
    const double c00 = (d * f) - (e * e), c01 = (cc * e) - (b * f), c02 = (b * e) - (cc * d);
    const double c11 = (a * f) - (cc * cc), c12 = (b * cc) - (a * e), c22 = (a * d) - (b * b);
    const double det = ((a * c00) + (b * c01)) + (cc * c02);
    if (det == 0.0 || det != det) return false;
    const double x0 = -(((c00 * g0) + (c01 * g1)) + (c02 * g2)) / det;
    const double x1 = -(((c01 * g0) + (c11 * g1)) + (c12 * g2)) / det;
    const double x2 = -(((c02 * g0) + (c12 * g1)) + (c22 * g2)) / det;
    if (!(fabs(x0) <= 1.0 && fabs(x1) <= 1.0 && fabs(x2) <= 1.0)) return false;
    const double half = o > 0 ? 0.5 : 0.0;   // an even window is centred half a pixel up-left of its sample
    K.x = ((double)j + x0) * (double)(1 << o) - half, K.y = ((double)i + x1) * (double)(1 << o) - half;
    K.size = (double)L + x2 * (double)(6 << o), K.response = v;
    return true;
}

// the sample a thread of block `blk` looks at: group g (block-uniform), row i, column j; false: padding of the group, or the margin
struct SfSample {
    int o, m, i, j, mw, L;
    const double *N0, *N1, *N2;
};
__device__ __forceinline__ bool sf_sample(const SurfArgs& A, int c, int blk, int tid, SfSample& S) {
    const int flat = blk * SF_T + tid;
    int g = 0;
    while (g + 1 < A.nGroups && flat >= A.grpStart[g + 1]) ++g;
    const int local = flat - A.grpStart[g], o = A.grpO[g], m = A.grpM[g], mw = A.mapW[o], mh = A.mapH[o], mg = A.grpMargin[g];
    if (local >= mw * mh) return false;
    const int i = local / mw, j = local - i * mw;
    if (i < mg || i >= mh - mg || j < mg || j >= mw - mg) return false;
    const double* base = A.det + (size_t)c * A.mapElems;
    const int ol = o * CS_SURF_MAX_LAYERS + m;
    S.o = o, S.m = m, S.i = i, S.j = j, S.mw = mw, S.L = A.layerSize[ol];
    S.N0 = base + A.mapOff[ol - 1], S.N1 = base + A.mapOff[ol], S.N2 = base + A.mapOff[ol + 1];
    return true;
}

__global__ __launch_bounds__(SF_T) void k_surf_maxima(SurfArgs A) {
    __shared__ int sCnt[SF_T / 64];
    const int c = blockIdx.y, blk = blockIdx.x, tid = threadIdx.x;
    bool key = false;
    SfSample S;
    if (A.img[c] && sf_sample(A, c, blk, tid, S)) {
        const int p = S.i * S.mw + S.j;
        const double v = S.N1[p];
        if (v > A.thr) {
            bool top = true;
            for (int di = -1; di <= 1; ++di)
                for (int dj = -1; dj <= 1; ++dj) {
                    const int q = p + di * S.mw + dj;
                    top = top && v > S.N0[q] && v > S.N2[q] && (q == p || v > S.N1[q]);
                }
            SfKey K;
            key = top && sf_newton(S.N0, S.N1, S.N2, S.mw, S.i, S.j, S.o, S.L, K);
        }
    }
    A.flag[(size_t)c * A.nFlat + (size_t)blk * SF_T + tid] = key ? 1 : 0;
    const sf_u64 bal = __ballot(key);
    if ((tid & 63) == 0) sCnt[tid >> 6] = __popcll(bal);
    __syncthreads();
    if (tid == 0) A.blockCnt[(size_t)c * A.nBlocks + blk] = (sCnt[0] + sCnt[1]) + (sCnt[2] + sCnt[3]);
}

// ---- the strongest-first choice (CS_SURF_KEEP_STRONGEST), between the maxima and the scan ---------------------------------------------
// A radix select over the candidates' responses, all cameras in each launch.  The first pass runs over every block: it counts the top 8
// bits of the keys and lists the blocks that hold a candidate (the WORK LIST; its order is the order of arrival and nothing reads it as
// an order).  The seven passes behind it, SF_SEL_GRID workgroups a camera over the work list, count the next 8 bits of the keys that share
// the cut's digits so far (integer atomics: the counts do not depend on the order of arrival); every workgroup reads the previous pass's
// 256 counts and settles that digit itself, so no pass waits for a deciding launch, and workgroup 0 of a camera stores what it settled for
// the next launch to start from.  Then the candidates AT the cut are counted per block, scanned, and the flags and block counts are
// rewritten: above the cut, or at it and among the first `need` in list order.  k_surf_scan / k_surf_scatter see a list of exactly
// maxPts.  A camera with total <= maxPts is left alone (need = 0 after the first pass).
constexpr int SF_SEL_GRID = 64;

// larger response <-> larger key, as unsigned integers (a candidate's response is above the threshold >= 0; the rule holds for any double)
__device__ __forceinline__ sf_u64 sf_key(double v) {
    const sf_u64 b = (sf_u64)__double_as_longlong(v);
    return (b >> 63) ? ~b : (b | (1ull << 63));
}

// the key of the thread's sample when it is flagged
__device__ __forceinline__ bool sf_candidate(const SurfArgs& A, int c, int blk, int tid, sf_u64& key) {
    SfSample S;
    if (!A.flag[(size_t)c * A.nFlat + (size_t)blk * SF_T + tid] || !sf_sample(A, c, blk, tid, S)) return false;
    key = sf_key(S.N1[S.i * S.mw + S.j]);
    return true;
}

__global__ __launch_bounds__(SF_T) void k_surf_sel_first(SurfArgs A) {
    const int c = blockIdx.y, blk = blockIdx.x, tid = threadIdx.x;
    if (!A.img[c] || A.blockCnt[(size_t)c * A.nBlocks + blk] == 0) return;   // (uniform)
    if (tid == 0) A.workList[(size_t)c * A.nBlocks + atomicAdd(&A.nWork[c], 1)] = blk;
    sf_u64 key;
    if (sf_candidate(A, c, blk, tid, key)) atomicAdd(&A.selHist[((size_t)c * SF_SEL_PASSES) * 256 + (int)(key >> 56)], 1u);
}

// The digit of pass p - 1 from its counts and the select in front of it: the digit d with fewer than `need` keys above it and at least
// `need` with its own.  The whole workgroup calls this (thread t owns digit t); every thread gets the result, workgroup 0 stores it.
__device__ SfSel sf_sel_decide(const SurfArgs& A, int c, int p) {
    __shared__ int sW[SF_T / 64];
    __shared__ SfSel sOut;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    SfSel st;
    if (p == 1)
        st.prefix = 0, st.need = A.maxPts, st.bin = 0;
    else
        st = A.selState[(size_t)c * (SF_SEL_PASSES + 1) + (p - 1)];
    if (st.need > 0) {   // (uniform)
        const int h = (int)A.selHist[((size_t)c * SF_SEL_PASSES + (p - 1)) * 256 + tid];
        int inc = h;
        for (int d = 1; d < 64; d <<= 1) {
            const int o = __shfl_up(inc, d, 64);
            if (lane >= d) inc += o;
        }
        if (lane == 63) sW[w] = inc;
        __syncthreads();
        for (int k = 0; k < w; ++k) inc += sW[k];
        const int total = (sW[0] + sW[1]) + (sW[2] + sW[3]), above = total - inc;
        if (tid == 0) sOut.prefix = st.prefix, sOut.need = 0, sOut.bin = 0;   // the first pass of a camera with total <= maxPts: no digit
        __syncthreads();
        if (!(p == 1 && total <= st.need) && above < st.need && above + h >= st.need)   // one thread
            sOut.prefix = st.prefix | ((sf_u64)tid << (64 - 8 * p)), sOut.need = st.need - above, sOut.bin = h;
        __syncthreads();
        st = sOut;
        if (p == 1 && tid == 0 && blockIdx.x == 0) A.dropped[c] = st.need > 0 ? total - A.maxPts : 0;
    }
    if (blockIdx.x == 0 && tid == 0) A.selState[(size_t)c * (SF_SEL_PASSES + 1) + p] = st;
    return st;
}

__global__ __launch_bounds__(SF_T) void k_surf_sel_hist(SurfArgs A, int p) {   // p = 1 .. SF_SEL_PASSES - 1
    const int c = blockIdx.y, tid = threadIdx.x;
    if (!A.img[c]) return;
    const SfSel st = sf_sel_decide(A, c, p);
    if (st.need <= 0) return;   // (uniform)
    const int nWork = A.nWork[c], shift = 56 - 8 * p;
    for (int w = blockIdx.x; w < nWork; w += SF_SEL_GRID) {
        sf_u64 key;
        if (sf_candidate(A, c, A.workList[(size_t)c * A.nBlocks + w], tid, key) && (key >> (shift + 8)) == (st.prefix >> (shift + 8)))
            atomicAdd(&A.selHist[((size_t)c * SF_SEL_PASSES + p) * 256 + (int)((key >> shift) & 255)], 1u);
    }
}

// the last digit, and the candidates AT the cut per block, only where some of them have to go (the other blocks' counts are the call's zeros)
__global__ __launch_bounds__(SF_T) void k_surf_sel_ties(SurfArgs A) {
    __shared__ int sCnt[SF_T / 64];
    const int c = blockIdx.y, tid = threadIdx.x;
    if (!A.img[c]) return;
    const SfSel st = sf_sel_decide(A, c, SF_SEL_PASSES);
    if (st.need <= 0 || st.bin == st.need) return;   // (uniform)
    const int nWork = A.nWork[c];
    for (int w = blockIdx.x; w < nWork; w += SF_SEL_GRID) {
        const int blk = A.workList[(size_t)c * A.nBlocks + w];
        sf_u64 key;
        const bool tie = sf_candidate(A, c, blk, tid, key) && key == st.prefix;
        const sf_u64 bal = __ballot(tie);
        if ((tid & 63) == 0) sCnt[tid >> 6] = __popcll(bal);
        __syncthreads();
        if (tid == 0) A.tieCnt[(size_t)c * A.nBlocks + blk] = (sCnt[0] + sCnt[1]) + (sCnt[2] + sCnt[3]);
        __syncthreads();
    }
}

__device__ int sf_scan_blocks(const int* cnt, int* off, int nB);   // (below, with k_surf_scan)

__global__ __launch_bounds__(SF_T) void k_surf_sel_tiescan(SurfArgs A) {
    const int c = blockIdx.x;
    if (!A.img[c]) return;
    const SfSel st = A.selState[(size_t)c * (SF_SEL_PASSES + 1) + SF_SEL_PASSES];
    if (st.need <= 0 || st.bin == st.need) return;   // (uniform)
    sf_scan_blocks(A.tieCnt + (size_t)c * A.nBlocks, A.tieOff + (size_t)c * A.nBlocks, A.nBlocks);
}

// the flags and block counts of the kept candidates: above the cut, or at it and among the first `need` of those in list order
__global__ __launch_bounds__(SF_T) void k_surf_sel_reflag(SurfArgs A) {
    __shared__ int sTie[SF_T / 64], sKeep[SF_T / 64];
    const int c = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    if (!A.img[c]) return;
    const SfSel st = A.selState[(size_t)c * (SF_SEL_PASSES + 1) + SF_SEL_PASSES];
    if (st.need <= 0) return;   // (uniform)
    const int nWork = A.nWork[c];
    for (int w = blockIdx.x; w < nWork; w += SF_SEL_GRID) {
        const int blk = A.workList[(size_t)c * A.nBlocks + w];
        sf_u64 key = 0;
        const bool cand = sf_candidate(A, c, blk, tid, key), tie = cand && key == st.prefix;
        const sf_u64 balT = __ballot(tie);
        if (lane == 0) sTie[wv] = __popcll(balT);
        __syncthreads();
        bool keep = cand && key > st.prefix;
        if (tie) {
            int rank = __popcll(balT & ((1ull << lane) - 1));
            for (int k = 0; k < wv; ++k) rank += sTie[k];
            keep = st.bin == st.need || A.tieOff[(size_t)c * A.nBlocks + blk] + rank < st.need;
        }
        if (cand && !keep) A.flag[(size_t)c * A.nFlat + (size_t)blk * SF_T + tid] = 0;
        const sf_u64 balK = __ballot(keep);
        if (lane == 0) sKeep[wv] = __popcll(balK);
        __syncthreads();
        if (tid == 0) A.blockCnt[(size_t)c * A.nBlocks + blk] = (sKeep[0] + sKeep[1]) + (sKeep[2] + sKeep[3]);
        __syncthreads();
    }
}

// ---- the order: an exclusive scan of the block counts per camera (one workgroup each), then every block places its own key points -----
// off[b] = cnt[0] + .. + cnt[b - 1] for the nB blocks of a camera, by one workgroup -> the total (in every thread)
__device__ int sf_scan_blocks(const int* cnt, int* off, int nB) {
    __shared__ int sW[SF_T / 64];
    __shared__ int sBase;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    if (tid == 0) sBase = 0;
    __syncthreads();
    for (int b0 = 0; b0 < nB; b0 += SF_T) {
        const int b = b0 + tid;
        const int v = b < nB ? cnt[b] : 0;
        int inc = v;
        for (int d = 1; d < 64; d <<= 1) {
            const int o = __shfl_up(inc, d, 64);
            if (lane >= d) inc += o;
        }
        if (lane == 63) sW[w] = inc;
        __syncthreads();
        int pre = sBase;
        for (int k = 0; k < w; ++k) pre += sW[k];
        if (b < nB) off[b] = pre + inc - v;
        __syncthreads();
        if (tid == 0) sBase += (sW[0] + sW[1]) + (sW[2] + sW[3]);
        __syncthreads();
    }
    return sBase;
}

__global__ __launch_bounds__(SF_T) void k_surf_scan(SurfArgs A) {
    const int c = blockIdx.x;
    const int total = sf_scan_blocks(A.blockCnt + (size_t)c * A.nBlocks, A.blockOff + (size_t)c * A.nBlocks, A.img[c] ? A.nBlocks : 0);
    if (threadIdx.x == 0) {
        const int n = total < A.maxPts ? total : A.maxPts;
        A.count[c] = n, A.overflow[c] = (total - n) + (A.dropped && A.img[c] ? A.dropped[c] : 0);
    }
}

__global__ __launch_bounds__(SF_T) void k_surf_scatter(SurfArgs A) {
    __shared__ int sCnt[SF_T / 64];
    const int c = blockIdx.y, blk = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    if (!A.img[c] || A.blockCnt[(size_t)c * A.nBlocks + blk] == 0) return;   // (uniform)
    const bool key = A.flag[(size_t)c * A.nFlat + (size_t)blk * SF_T + tid] != 0;
    const sf_u64 bal = __ballot(key);
    if (lane == 0) sCnt[w] = __popcll(bal);
    __syncthreads();
    int pos = A.blockOff[(size_t)c * A.nBlocks + blk] + __popcll(bal & ((1ull << lane) - 1));
    for (int k = 0; k < w; ++k) pos += sCnt[k];
    if (!key || pos >= A.maxPts) return;
    SfSample S;
    SfKey K;
    if (!sf_sample(A, c, blk, tid, S) || !sf_newton(S.N0, S.N1, S.N2, S.mw, S.i, S.j, S.o, S.L, K)) return;   // (cannot be: it was flagged)
    const size_t at = (size_t)c * A.maxPts + pos;
    A.pts[2 * at] = K.x, A.pts[2 * at + 1] = K.y, A.size[at] = K.size, A.response[at] = K.response, A.angle[at] = 0.0;
    A.laplacian[at] = A.lap[(size_t)c * A.mapElems + A.mapOff[S.o * CS_SURF_MAX_LAYERS + S.m] + S.i * S.mw + S.j];
    A.octave[at] = S.o, A.layer[at] = S.m, A.cell[2 * at] = S.i, A.cell[2 * at + 1] = S.j;
    for (int k = 0; k < A.dim; ++k) A.desc[at * A.dim + k] = 0.0f;
}

// rows >= count: NaN key points, zero descriptors
__global__ __launch_bounds__(SF_T) void k_surf_pad(SurfArgs A) {
    const int c = blockIdx.y, k = blockIdx.x * SF_T + threadIdx.x;
    if (k >= A.maxPts || k < A.count[c]) return;
    const size_t at = (size_t)c * A.maxPts + k;
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    A.pts[2 * at] = nan, A.pts[2 * at + 1] = nan, A.size[at] = nan, A.response[at] = nan, A.angle[at] = nan;
    A.laplacian[at] = 0, A.octave[at] = 0, A.layer[at] = 0, A.cell[2 * at] = 0, A.cell[2 * at + 1] = 0;
    for (int d = 0; d < A.dim; ++d) A.desc[at * A.dim + d] = 0.0f;
}

// ---- orientation: a wave per key point; lanes over the 109 samples, then over the 72 windows ------------------------------------------
__global__ __launch_bounds__(SF_T) void k_surf_orient(SurfArgs A) {
    __shared__ double sRx[SF_T / 64][SF_ORI], sRy[SF_T / 64][SF_ORI], sAng[SF_T / 64][SF_ORI];
    __shared__ double sScore[SF_T / 64][SF_WIN], sSx[SF_T / 64][SF_WIN], sSy[SF_T / 64][SF_WIN];
    const int c = blockIdx.y, tid = threadIdx.x, lane = tid & 63, w = tid >> 6, kp = blockIdx.x * (SF_T / 64) + w;
    const bool on = A.img[c] && kp < A.count[c];      // (no early return: the barriers below are the workgroup's)
    const size_t at = (size_t)c * A.maxPts + (on ? kp : 0);
    const double x = A.pts[2 * at], y = A.pts[2 * at + 1], s = (1.2 * A.size[at]) / 9.0;
    const unsigned* I = sf_integral(A, c);
    if (on) {
        int h = sf_round(4.0 * s);
        h = h < 2 ? 2 : h;
        for (int k = lane; k < SF_ORI; k += 64) {
            const int px = sf_round(x + A.oriGrid[2 * k] * s), py = sf_round(y + A.oriGrid[2 * k + 1] * s);
            long long hx, hy;
            sf_haar(I, A.W, A.H, py, px, h, hx, hy);
            const double wk = A.oriW[k], rx = wk * (double)hx, ry = wk * (double)hy;
            double ang = atan2(ry, rx);
            if (ang < 0.0) ang += SF_TWO_PI;
            sRx[w][k] = rx, sRy[w][k] = ry, sAng[w][k] = ang;
        }
    }
    __syncthreads();
    if (on) {
        for (int wd = lane; wd < SF_WIN; wd += 64) {
            const double a0 = ((double)wd + 0.5) * SF_WIN_STEP;   // (no edge on a multiple of 45 degrees, where integer responses put angles exactly)
            double sx = 0.0, sy = 0.0;
            for (int k = 0; k < SF_ORI; ++k) {
                const double rx = sRx[w][k], ry = sRy[w][k];
                double d = sAng[w][k] - a0;
                if (d < 0.0) d += SF_TWO_PI;
                if ((rx != 0.0 || ry != 0.0) && d < SF_WIN_WIDTH) sx += rx, sy += ry;
            }
            sSx[w][wd] = sx, sSy[w][wd] = sy, sScore[w][wd] = (sx * sx) + (sy * sy);
        }
    }
    __syncthreads();
    if (on && lane == 0) {
        int best = 0;
        for (int wd = 1; wd < SF_WIN; ++wd)
            if (sScore[w][wd] > sScore[w][best]) best = wd;   // the lowest index of equals
        A.angle[at] = atan2(sSy[w][best], sSx[w][best]);
    }
}

// ---- descriptor: a wave per key point, four lanes per subregion ------------------------------------------------------------------------
template <int DIM>
__global__ __launch_bounds__(SF_T) void k_surf_describe(SurfArgs A, int upright) {
    constexpr int NC = DIM / 16;   // components of a subregion: 4 or 8
    __shared__ double sVec[SF_T / 64][DIM];
    __shared__ double sNorm[SF_T / 64];
    const int c = blockIdx.y, tid = threadIdx.x, lane = tid & 63, w = tid >> 6, kp = blockIdx.x * (SF_T / 64) + w;
    const bool on = A.img[c] && kp < A.count[c];
    const size_t at = (size_t)c * A.maxPts + (on ? kp : 0);
    const double x = A.pts[2 * at], y = A.pts[2 * at + 1], s = (1.2 * A.size[at]) / 9.0, th = A.angle[at];
    const double co = upright ? 1.0 : cos(th), si = upright ? 0.0 : sin(th);
    const unsigned* I = sf_integral(A, c);
    const int sub = lane >> 2, q = lane & 3;
    double acc[NC];
#pragma unroll
    for (int k = 0; k < NC; ++k) acc[k] = 0.0;
    if (on) {
        int h = sf_round(2.0 * s);
        h = h < 2 ? 2 : h;
        for (int t = q; t < 25; t += 4) {
            const int a = (sub & 3) * 5 + t % 5, b = (sub >> 2) * 5 + t / 5;
            const double u = (double)a - 9.5, v = (double)b - 9.5;
            const int px = sf_round(x + ((u * co) - (v * si)) * s), py = sf_round(y + ((u * si) + (v * co)) * s);
            long long hx, hy;
            sf_haar(I, A.W, A.H, py, px, h, hx, hy);
            const double g = A.descW[b * 20 + a], rx = g * (double)hx, ry = g * (double)hy;
            const double tdx = (co * rx) + (si * ry), tdy = (co * ry) - (si * rx);
            if constexpr (NC == 4) {
                acc[0] += tdx, acc[1] += tdy, acc[2] += fabs(tdx), acc[3] += fabs(tdy);
            } else {
                const bool ny = tdy < 0.0, nx = tdx < 0.0;
                acc[0] += ny ? tdx : 0.0, acc[1] += ny ? 0.0 : tdx, acc[2] += ny ? fabs(tdx) : 0.0, acc[3] += ny ? 0.0 : fabs(tdx);
                acc[4] += nx ? tdy : 0.0, acc[5] += nx ? 0.0 : tdy, acc[6] += nx ? fabs(tdy) : 0.0, acc[7] += nx ? 0.0 : fabs(tdy);
            }
        }
    }
#pragma unroll
    for (int k = 0; k < NC; ++k) {   // (p0 + p1) + (p2 + p3) in every lane of the four
        acc[k] += cs_shfl_xor_d(acc[k], 1);
        acc[k] += cs_shfl_xor_d(acc[k], 2);
    }
    if (q == 0) {
#pragma unroll
        for (int k = 0; k < NC; ++k) sVec[w][sub * NC + k] = acc[k];
    }
    __syncthreads();
    if (lane == 0) {
        double ss = 0.0;
        for (int k = 0; k < DIM; ++k) ss += sVec[w][k] * sVec[w][k];   // in index order
        sNorm[w] = sqrt(ss);
    }
    __syncthreads();
    if (!on) return;
    const double norm = sNorm[w];
    const bool none = norm == 0.0 || norm != norm;
    for (int k = lane; k < DIM; k += 64) A.desc[at * DIM + k] = none ? 0.0f : (float)(sVec[w][k] / norm);
    if (none && lane == 0) {
        const double nan = __longlong_as_double(0x7ff8000000000000ll);
        A.pts[2 * at] = nan, A.pts[2 * at + 1] = nan;
    }
}

}  // namespace

struct cs_surf {
    int device;
    char* base;
    size_t bytes;
    cs_surf_buffers b;
    SurfArgs args;      // the tables; img, pitch and thr are the call's
    double *oriW, *oriGrid, *descW;
    int maxMap;         // samples of the largest layer map
    int keep;           // CS_SURF_KEEP_FIRST | CS_SURF_KEEP_STRONGEST
    CsStage stage;
};

// the device block: the tables, per camera the integral image, the maps, the flags and block tables, the key-point arrays
static void sf_layout(cs_surf* sf, CsArena& ar) {
    SurfArgs& A = sf->args;
    const size_t nC = (size_t)sf->b.nCams, nP = nC * A.maxPts;
    ar.take(sf->oriW, SF_ORI), ar.take(sf->oriGrid, 2 * SF_ORI), ar.take(sf->descW, 400);
    ar.take(A.integral, nC * (size_t)(A.H + 1) * (size_t)(A.W + 1)), ar.take(A.det, nC * A.mapElems), ar.take(A.lap, nC * A.mapElems);
    ar.take(A.flag, nC * A.nFlat), ar.take(A.blockCnt, nC * A.nBlocks), ar.take(A.blockOff, nC * A.nBlocks);
    ar.take(A.pts, nP * 2), ar.take(A.desc, nP * A.dim), ar.take(A.size, nP), ar.take(A.angle, nP), ar.take(A.response, nP);
    ar.take(A.laplacian, nP), ar.take(A.octave, nP), ar.take(A.layer, nP), ar.take(A.cell, nP * 2), ar.take(A.count, nC), ar.take(A.overflow, nC);
    ar.take(A.selHist, nC * SF_SEL_PASSES * 256), ar.take(A.nWork, nC), ar.take(A.tieCnt, nC * A.nBlocks);   // (zeroed as one range)
    ar.take(A.tieOff, nC * A.nBlocks), ar.take(A.workList, nC * A.nBlocks), ar.take(A.selState, nC * (SF_SEL_PASSES + 1)), ar.take(A.dropped, nC);
}

extern "C" cs_surf* cs_surf_create(int device, int nCams, int W, int H, int maxPts, int nOctaves, int nOctaveLayers, int dimDesc) {
    if (nCams < 1 || nCams > SF_MAX_CAMS || W < 1 || H < 1 || maxPts < 1 || maxPts > SF_MAX_PTS || nOctaves < 1 || nOctaves > CS_SURF_MAX_OCTAVES ||
        nOctaveLayers < 1 || nOctaveLayers > CS_SURF_MAX_LAYERS - 2 || (dimDesc != 64 && dimDesc != 128)) {
        cs_set_error("cs_surf_create: bad argument (nCams %d of 1..%d, W %d, H %d, maxPts %d of 1..%d, nOctaves %d of 1..%d, nOctaveLayers %d of 1..%d, dimDesc %d of 64 | 128)",
                     nCams, SF_MAX_CAMS, W, H, maxPts, SF_MAX_PTS, nOctaves, CS_SURF_MAX_OCTAVES, nOctaveLayers, CS_SURF_MAX_LAYERS - 2, dimDesc);
        return nullptr;
    }
    if ((unsigned long long)W * (unsigned long long)H * 255ull >= (1ull << 32)) {
        cs_set_error("cs_surf_create: W %d x H %d: W H 255 >= 2^32, the integral image is 32 bits", W, H);
        return nullptr;
    }
    cs_surf* sf = new cs_surf();
    sf->device = device, sf->base = nullptr, sf->bytes = 0, sf->maxMap = 0, sf->keep = CS_SURF_KEEP_FIRST;
    SurfArgs& A = sf->args;
    memset(&A, 0, sizeof(A));
    cs_surf_buffers& B = sf->b;
    memset(&B, 0, sizeof(B));
    A.W = W, A.H = H, A.maxPts = maxPts, A.nOct = nOctaves, A.nLay = nOctaveLayers, A.dim = dimDesc;
    const int minWH = W < H ? W : H;
    for (int k = 0; k < SF_NL; ++k) A.mapOff[k] = -1;
    for (int o = 0; o < nOctaves; ++o) {
        A.mapW[o] = W >> o, A.mapH[o] = H >> o;
        const int n = A.mapW[o] * A.mapH[o];
        sf->maxMap = n > sf->maxMap ? n : sf->maxMap;
        for (int l = 0; l < nOctaveLayers + 2; ++l) {
            const int ol = o * CS_SURF_MAX_LAYERS + l;
            A.layerSize[ol] = (9 + 6 * l) << o, A.layerFits[ol] = A.layerSize[ol] < minWH ? 1 : 0;
            A.mapOff[ol] = A.mapElems, A.mapElems += n;
        }
        for (int m = 1; m <= nOctaveLayers; ++m) {   // a group: a middle layer whose upper neighbour fits and whose margin leaves samples
            const int ol = o * CS_SURF_MAX_LAYERS + m, mg = ((A.layerSize[ol + 1] / 2) >> o) + 1;
            if (!A.layerFits[ol + 1] || A.mapH[o] - 2 * mg <= 0 || A.mapW[o] - 2 * mg <= 0) continue;
            const int g = A.nGroups++;
            A.grpO[g] = o, A.grpM[g] = m, A.grpMargin[g] = mg, A.grpStart[g + 1] = A.grpStart[g] + (n + SF_T - 1) / SF_T * SF_T;
        }
    }
    A.nFlat = A.grpStart[A.nGroups], A.nBlocks = A.nFlat / SF_T;
    B.nCams = nCams;
    if (!cs_arena_alloc(device, sf->base, sf->bytes, [sf](CsArena& ar) { sf_layout(sf, ar); })) {
        cs_set_error("cs_surf_create: %zu bytes of device memory: %s", sf->bytes, hipGetErrorString(hipGetLastError()));
        delete sf;
        return nullptr;
    }
    // the weight tables, built on the host: sigma = 2 s over the 109 orientation samples (i outer, j inner), 3.3 s over the 20 x 20 window
    double oriW[SF_ORI], oriGrid[2 * SF_ORI], descW[400];
    int k = 0;
    for (int i = -6; i <= 6; ++i)
        for (int j = -6; j <= 6; ++j)
            if (i * i + j * j < 36) oriGrid[2 * k] = i, oriGrid[2 * k + 1] = j, oriW[k] = exp(-(double)(i * i + j * j) / 8.0), ++k;
    for (int b = 0; b < 20; ++b)
        for (int a = 0; a < 20; ++a) descW[b * 20 + a] = exp(-((a - 9.5) * (a - 9.5) + (b - 9.5) * (b - 9.5)) / (2.0 * 3.3 * 3.3));
    if (sf->stage.begin(nullptr) != CS_OK || sf->stage.upload(nullptr, sf->oriW, oriW, sizeof(oriW)) != CS_OK ||
        sf->stage.upload(nullptr, sf->oriGrid, oriGrid, sizeof(oriGrid)) != CS_OK || sf->stage.upload(nullptr, sf->descW, descW, sizeof(descW)) != CS_OK) {
        cs_surf_destroy(sf);
        return nullptr;
    }
    sf->stage.drain();   // the tables are in place before the first call, on whatever stream that runs: no call of the handle waits
    A.oriW = sf->oriW, A.oriGrid = sf->oriGrid, A.descW = sf->descW;
    B.pts = A.pts, B.desc = A.desc, B.size = A.size, B.angle = A.angle, B.response = A.response, B.laplacian = A.laplacian, B.octave = A.octave;
    B.layer = A.layer, B.cell = A.cell, B.count = A.count, B.overflow = A.overflow, B.integral = A.integral, B.det = A.det, B.lap = A.lap;
    B.W = W, B.H = H, B.maxPts = maxPts, B.nOctaves = nOctaves, B.nOctaveLayers = nOctaveLayers, B.dimDesc = dimDesc, B.mapElems = A.mapElems;
    memcpy(B.mapW, A.mapW, sizeof(B.mapW)), memcpy(B.mapH, A.mapH, sizeof(B.mapH)), memcpy(B.mapOff, A.mapOff, sizeof(B.mapOff));
    memcpy(B.layerSize, A.layerSize, sizeof(B.layerSize)), memcpy(B.layerFits, A.layerFits, sizeof(B.layerFits));
    return sf;
}

extern "C" void cs_surf_destroy(cs_surf* sf) {
    if (!sf) return;
    if (sf->base) {
        (void)hipSetDevice(sf->device);
        sf->stage.drain();
        (void)hipFree(sf->base);
    }
    delete sf;
}

namespace {

enum { SF_INTEGRAL = 0, SF_LAYERS = 1, SF_DETECT = 2, SF_ALL = 3 };

int sf_run(const char* who, cs_surf* sf, void* hip_stream, const unsigned char* const* d_img, int pitch, double thr, int upright, int upTo) {
    if (!sf || !d_img) {
        cs_set_error("%s: null handle or image table", who);
        return CS_ERR_INVALID;
    }
    if (pitch < sf->args.W) {
        cs_set_error("%s: pitch %d below the width %d", who, pitch, sf->args.W);
        return CS_ERR_INVALID;
    }
    if (!(thr >= 0.0) || !std::isfinite(thr)) {
        cs_set_error("%s: the threshold %g is negative or not finite", who, thr);
        return CS_ERR_INVALID;
    }
    SurfArgs A = sf->args;
    const int nC = sf->b.nCams;
    const bool strongest = sf->keep == CS_SURF_KEEP_STRONGEST && A.nBlocks > 0;
    if (!strongest) A.dropped = nullptr;   // what k_surf_scan adds to the overflow
    for (int c = 0; c < nC; ++c) A.img[c] = d_img[c];
    A.pitch = pitch, A.thr = thr;
    hipStream_t s = (hipStream_t)hip_stream;
    CS_HIP(hipSetDevice(sf->device));
    hipLaunchKernelGGL(k_surf_rows, dim3(A.H, nC), dim3(64), 0, s, A);
    CS_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_surf_cols, dim3((A.W + 1 + SF_T - 1) / SF_T, nC), dim3(SF_T), 0, s, A);
    CS_CHECK_LAUNCH();
    if (upTo == SF_INTEGRAL) return CS_OK;
    hipLaunchKernelGGL(k_surf_response, dim3((sf->maxMap + SF_T - 1) / SF_T, A.nOct * CS_SURF_MAX_LAYERS, nC), dim3(SF_T), 0, s, A);
    CS_CHECK_LAUNCH();
    if (upTo == SF_LAYERS) return CS_OK;
    if (A.nBlocks > 0) {
        hipLaunchKernelGGL(k_surf_maxima, dim3(A.nBlocks, nC), dim3(SF_T), 0, s, A);
        CS_CHECK_LAUNCH();
    }
    if (strongest) {
        CS_HIP(hipMemsetAsync(A.selHist, 0, (size_t)((char*)(A.tieCnt + (size_t)nC * A.nBlocks) - (char*)A.selHist), s));
        hipLaunchKernelGGL(k_surf_sel_first, dim3(A.nBlocks, nC), dim3(SF_T), 0, s, A);
        CS_CHECK_LAUNCH();
        for (int p = 1; p < SF_SEL_PASSES; ++p) {
            hipLaunchKernelGGL(k_surf_sel_hist, dim3(SF_SEL_GRID, nC), dim3(SF_T), 0, s, A, p);
            CS_CHECK_LAUNCH();
        }
        hipLaunchKernelGGL(k_surf_sel_ties, dim3(SF_SEL_GRID, nC), dim3(SF_T), 0, s, A);
        CS_CHECK_LAUNCH();
        hipLaunchKernelGGL(k_surf_sel_tiescan, dim3(nC), dim3(SF_T), 0, s, A);
        CS_CHECK_LAUNCH();
        hipLaunchKernelGGL(k_surf_sel_reflag, dim3(SF_SEL_GRID, nC), dim3(SF_T), 0, s, A);
        CS_CHECK_LAUNCH();
    }
    hipLaunchKernelGGL(k_surf_scan, dim3(nC), dim3(SF_T), 0, s, A);
    CS_CHECK_LAUNCH();
    if (A.nBlocks > 0) {
        hipLaunchKernelGGL(k_surf_scatter, dim3(A.nBlocks, nC), dim3(SF_T), 0, s, A);
        CS_CHECK_LAUNCH();
    }
    hipLaunchKernelGGL(k_surf_pad, dim3((A.maxPts + SF_T - 1) / SF_T, nC), dim3(SF_T), 0, s, A);
    CS_CHECK_LAUNCH();
    if (upTo == SF_DETECT || A.nBlocks == 0) return CS_OK;
    const dim3 perKey((A.maxPts + SF_T / 64 - 1) / (SF_T / 64), nC);
    if (!upright) {
        hipLaunchKernelGGL(k_surf_orient, perKey, dim3(SF_T), 0, s, A);
        CS_CHECK_LAUNCH();
    }
    if (A.dim == 64)
        hipLaunchKernelGGL(k_surf_describe<64>, perKey, dim3(SF_T), 0, s, A, upright ? 1 : 0);
    else
        hipLaunchKernelGGL(k_surf_describe<128>, perKey, dim3(SF_T), 0, s, A, upright ? 1 : 0);
    CS_CHECK_LAUNCH();
    return CS_OK;
}

}  // namespace

extern "C" int cs_surf_run_dev(cs_surf* sf, void* hip_stream, const unsigned char* const* d_img, int pitch, double hessianThreshold, int upright) {
    return sf_run("cs_surf_run_dev", sf, hip_stream, d_img, pitch, hessianThreshold, upright, SF_ALL);
}

extern "C" int cs_surf_integral_dev(cs_surf* sf, void* hip_stream, const unsigned char* const* d_img, int pitch) {
    return sf_run("cs_surf_integral_dev", sf, hip_stream, d_img, pitch, 0.0, 1, SF_INTEGRAL);
}

extern "C" int cs_surf_layers_dev(cs_surf* sf, void* hip_stream, const unsigned char* const* d_img, int pitch) {
    return sf_run("cs_surf_layers_dev", sf, hip_stream, d_img, pitch, 0.0, 1, SF_LAYERS);
}

extern "C" int cs_surf_detect_dev(cs_surf* sf, void* hip_stream, const unsigned char* const* d_img, int pitch, double hessianThreshold) {
    return sf_run("cs_surf_detect_dev", sf, hip_stream, d_img, pitch, hessianThreshold, 1, SF_DETECT);
}

extern "C" int cs_surf_keep_set(cs_surf* sf, int keep) {
    if (!sf || (keep != CS_SURF_KEEP_FIRST && keep != CS_SURF_KEEP_STRONGEST)) {
        cs_set_error("cs_surf_keep_set: null handle, or keep %d is neither CS_SURF_KEEP_FIRST nor CS_SURF_KEEP_STRONGEST", keep);
        return CS_ERR_INVALID;
    }
    sf->keep = keep;
    return CS_OK;
}

extern "C" int cs_surf_counts(cs_surf* sf, void* hip_stream, int* count, int* overflow) {
    if (!sf) {
        cs_set_error("cs_surf_counts: null handle");
        return CS_ERR_INVALID;
    }
    hipStream_t s = (hipStream_t)hip_stream;
    CS_HIP(hipSetDevice(sf->device));
    const size_t n = sizeof(int) * (size_t)sf->b.nCams;
    if (count) CS_HIP(hipMemcpyAsync(count, sf->b.count, n, hipMemcpyDeviceToHost, s));
    if (overflow) CS_HIP(hipMemcpyAsync(overflow, sf->b.overflow, n, hipMemcpyDeviceToHost, s));
    CS_HIP(hipStreamSynchronize(s));
    return CS_OK;
}

extern "C" int cs_surf_buffers_get(const cs_surf* sf, cs_surf_buffers* out) {
    if (!sf || !out) {
        cs_set_error("cs_surf_buffers_get: bad arguments");
        return CS_ERR_INVALID;
    }
    *out = sf->b;
    return CS_OK;
}

extern "C" int cs_surf_download(cs_surf* sf, void* hip_stream, const void* d_src, void* h_dst, size_t bytes) {
    return cs_arena_download("cs_surf_download", sf ? sf->device : 0, sf ? sf->base : nullptr, sf ? sf->bytes : 0, hip_stream, d_src, h_dst, bytes);
}
