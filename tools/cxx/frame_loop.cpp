// frame_loop.cpp -- the headline frame loop of bench.py driven from C++ through the C-ABI only (include/coslam_hip.h): no
// Python, no torch.  north_star: "Host stays C++".  Same workload, same streams, same key-frame cadence, same drain as
// bench.py's timed loop; the workload (synthetic frames, map, BA problems, pose graphs) is read from the file bench.py writes
// with --export-workload (tools: bench.py export_workload()).
//   hipcc -O2 -std=c++17 -Iinclude tools/cxx/frame_loop.cpp -Lcoslam_amd/lib -lcoslam_hip -Wl,-rpath,$PWD/coslam_amd/lib \
//         -o tools/cxx/frame_loop.bin
//   tools/cxx/frame_loop.bin <workload file> <steps> <warmup> [cams per tracker launch] [BA apply lag in key-frame intervals: 2]
//                            [first timed frame: 0]
// Environment (read once, by read_options): RANK / WORLD_SIZE / LOCAL_RANK, COSLAM_FORCE_DEVICE, COSLAM_COMM, COSLAM_COMM_ID_FILE
// (ranks); COSLAM_KLT_FUSED=0 (the launch-per-pass tracker); COSLAM_FUSED_ROUNDS=0 (the launch-per-step registration);
// COSLAM_PIXEL_ERR_STD=1; COSLAM_KEYFRAME_DRIVES=1, COSLAM_KEYFRAME_LAG, COSLAM_KEYFRAME_RATIO (the key-frame decision);
// COSLAM_EXPORT_DIR (the run's result files, written there after the drain: cs_loop_export_results) with COSLAM_EXPORT_FRAMES (the
// whole-run archive behind the pose history, in frames: cs_track_history_set_archive); COSLAM_HIST_STORE (frames of pixels + poses the pose
// history keeps: 4096, as LoopConfig.hist_store); COSLAM_CAMERA_GROUPING=1 (CoSLAM::cameraGrouping per frame behind the pose update, reported
// under "camera_grouping": cs_camera_grouping_dev) with COSLAM_GROUP_MIN_OVERLAP_NUM (0), COSLAM_GROUP_MIN_AREA_RATIO (0.0),
// COSLAM_GROUP_MAX_DIST_RATIO (6.0); COSLAM_MERGE_CHECK=1 (MergeCameraGroup::checkPossibleMergable at every key frame over that frame's group
// record, reported under "merge_check": cs_merge_check_dev; needs COSLAM_CAMERA_GROUPING=1) with COSLAM_MERGE_MIN_IN_NUM (10),
// COSLAM_MERGE_MIN_AREA_RATIO (0.5), COSLAM_MERGE_MAX_CAM_DIST (6.0); COSLAM_LIVE_VIEW=1 (the frame's last step, cs_liveview_frame_dev: the counts, the dynamic points and
// every COSLAM_LIVE_VIEW_EVERY-th (1) frame a snapshot, reported under "live_view") with COSLAM_LIVE_VIEW_DEPTH (8), COSLAM_LIVE_VIEW_TRAIL_DEPTH
// (150), COSLAM_LIVE_VIEW_CUR_CAP / COSLAM_LIVE_VIEW_DYN_CAP (0: the map's capacity / a quarter of it).
// Per frame (reference call sites in bench.py's docstring): camera-group redetect (+ prefetch of the next frame's front) on the
// tracker stream; hand-back + intraCamEstimate of all cameras + both registration passes on the pose stream, event-ordered
// behind the tracker; at key frames the inter-camera solve and the joint local BA (parsed on the device from the window ring) on their
// workspaces' worker threads; `lag` key-frame intervals behind its key frame every joint BA's packed result is written back into
// the LIVE map, the pose history and the window (cs_ba_output_apply_dev = RobustBundleRTS::output(): key poses, points, outlier
// points false, relaxation of the non-key frames, updateNewPosesPoints) -- the pose stream waits for the record on the device.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

#include "coslam_hip.h"

#define HIPCHK(x)                                                                              \
    do {                                                                                       \
        hipError_t e_ = (x);                                                                   \
        if (e_ != hipSuccess) {                                                                \
            fprintf(stderr, "%s failed: %s (%s:%d)\n", #x, hipGetErrorString(e_), __FILE__, __LINE__); \
            exit(2);                                                                           \
        }                                                                                      \
    } while (0)
#define CSCHK(x)                                                                     \
    do {                                                                             \
        int rc_ = (x);                                                               \
        if (rc_ != CS_OK) {                                                          \
            fprintf(stderr, "%s failed (%d): %s (%s:%d)\n", #x, rc_, cs_last_error(), __FILE__, __LINE__); \
            exit(3);                                                                 \
        }                                                                            \
    } while (0)

// a handle the library returned, or exit 3 with its error
template <class T>
static T* made(T* p, const char* what) {
    if (!p) {
        fprintf(stderr, "%s: %s\n", what, cs_last_error());
        exit(3);
    }
    return p;
}

struct Reader {
    FILE* f;
    template <class T>
    std::vector<T> vec(size_t n) {
        std::vector<T> v(n);
        if (n && fread(v.data(), sizeof(T), n, f) != n) {
            fprintf(stderr, "workload file truncated\n");
            exit(4);
        }
        return v;
    }
    template <class T>
    void skip(size_t n) { (void)vec<T>(n); }
    int i32() { return vec<int>(1)[0]; }
    double f64() { return vec<double>(1)[0]; }
};

template <class T>
static T* to_dev(const std::vector<T>& h) {
    T* d = nullptr;
    HIPCHK(hipMalloc((void**)&d, sizeof(T) * (h.size() ? h.size() : 1)));
    if (!h.empty()) HIPCHK(hipMemcpy(d, h.data(), sizeof(T) * h.size(), hipMemcpyHostToDevice));
    return d;
}
template <class T>
static T* dev_zeros(size_t n) {
    T* d = nullptr;
    HIPCHK(hipMalloc((void**)&d, sizeof(T) * (n ? n : 1)));
    HIPCHK(hipMemset(d, 0, sizeof(T) * (n ? n : 1)));
    return d;
}

// ---- options: the command line and every environment variable the loop honours, read before any HIP call ----
struct Options {
    const char* workload;
    int steps, warmup;
    int camsPerLaunch;   // -1: the workload's
    int baLag;
    // the frame at which the timed region starts (bench.py hands over its own: both loops then time the SAME stretch of the sequence -- the
    // first hundreds of frames, while the map settles, are heavier than the steady state); 0: right behind the set-up
    int timedFrom;
    // One process per GPU (RANK / WORLD_SIZE / LOCAL_RANK as torch.distributed.run sets them; none: one rank).  COSLAM_FORCE_DEVICE: ranks
    // sharing one GPU (tests).  COSLAM_COMM=host:<segment>: the library's test transport; otherwise RCCL, the unique id through
    // COSLAM_COMM_ID_FILE
    int world, rank, dev;
    const char* hostSegment;   // nullptr: RCCL
    const char* commIdFile;
    bool kltFused;      // COSLAM_KLT_FUSED=0: the launch-per-pass tracker (two processes' persistent trackers on one GPU need not be co-resident)
    bool fusedRounds;   // COSLAM_FUSED_ROUNDS=0: the launch-per-step registration, the reference the fused launches are compared against
    bool pixIsStd;      // COSLAM_PIXEL_ERR_STD=1 (see PIXVAR below)
    bool kfDrives;      // COSLAM_KEYFRAME_DRIVES=1 (see KeyFrameDecision)
    int kfLag;
    double kfRatio;
    const char* exportDir;   // COSLAM_EXPORT_DIR: nullptr = no export
    int exportFrames;        // COSLAM_EXPORT_FRAMES: the archive's capacity (0: none)
    int histStore;           // COSLAM_HIST_STORE: frames the pose history keeps (>= the walks' 64)
    bool grouping;           // COSLAM_CAMERA_GROUPING=1 (see FrameLoop::camera_grouping)
    int groupMinNum;         // getViewOverlapCosts(viewOverlapCost, 0, 0.0), src/app/SL_CoSLAM.cpp:1635
    double groupMinAreaRatio, groupMaxDistRatio;   // Param::maxDistRatio = 6.0 (src/app/SL_GlobParam.cpp:18)
    bool mergeCheck;         // COSLAM_MERGE_CHECK=1 (see FrameLoop::merge_check)
    int mergeMinInNum;       // checkPossibleMergable(10, 0.5, Param::maxDistRatio), src/app/SL_CoSLAM.cpp:1380
    double mergeMinAreaRatio, mergeMaxCamDist;
    bool liveView;           // COSLAM_LIVE_VIEW=1 (see FrameLoop::live_view)
    int liveEvery, liveDepth, liveTrailDepth, liveCurCap, liveDynCap;
};

static Options read_options(int argc, char** argv) {
    if (argc < 4) {
        fprintf(stderr, "usage: %s <workload file> <steps> <warmup> [cams per tracker launch] [BA apply lag in key-frame intervals: 2] [first timed frame]\n", argv[0]);
        exit(1);
    }
    auto envi = [](const char* k, int dflt) { const char* e = getenv(k); return e && e[0] ? atoi(e) : dflt; };
    auto flag = [](const char* k, char on) { const char* e = getenv(k); return e && e[0] == on; };
    Options o;
    o.workload = argv[1];
    o.steps = atoi(argv[2]), o.warmup = atoi(argv[3]);
    o.camsPerLaunch = argc > 4 ? atoi(argv[4]) : -1;
    o.baLag = argc > 5 && atoi(argv[5]) > 0 ? atoi(argv[5]) : 2;
    o.timedFrom = argc > 6 ? atoi(argv[6]) : 0;
    o.world = envi("WORLD_SIZE", 1), o.rank = envi("RANK", 0);
    o.dev = envi("COSLAM_FORCE_DEVICE", envi("LOCAL_RANK", 0));
    const char* how = getenv("COSLAM_COMM");
    o.hostSegment = how && !strncmp(how, "host:", 5) ? how + 5 : nullptr;
    o.commIdFile = getenv("COSLAM_COMM_ID_FILE");
    o.kltFused = !flag("COSLAM_KLT_FUSED", '0');
    o.fusedRounds = !flag("COSLAM_FUSED_ROUNDS", '0');
    o.pixIsStd = flag("COSLAM_PIXEL_ERR_STD", '1');
    o.kfDrives = flag("COSLAM_KEYFRAME_DRIVES", '1');
    o.kfLag = std::max(1, envi("COSLAM_KEYFRAME_LAG", 1));
    const char* ratio = getenv("COSLAM_KEYFRAME_RATIO");
    o.kfRatio = ratio ? atof(ratio) : 0.93;   // m_mappedPtsReduceRatio
    const char* ed = getenv("COSLAM_EXPORT_DIR");
    o.exportDir = ed && ed[0] ? ed : nullptr;
    o.exportFrames = std::max(0, envi("COSLAM_EXPORT_FRAMES", 0));
    o.histStore = std::max(64, envi("COSLAM_HIST_STORE", 4096));
    o.grouping = flag("COSLAM_CAMERA_GROUPING", '1');
    o.groupMinNum = envi("COSLAM_GROUP_MIN_OVERLAP_NUM", 0);
    const char* gar = getenv("COSLAM_GROUP_MIN_AREA_RATIO");
    o.groupMinAreaRatio = gar && gar[0] ? atof(gar) : 0.0;
    const char* gdr = getenv("COSLAM_GROUP_MAX_DIST_RATIO");
    o.groupMaxDistRatio = gdr && gdr[0] ? atof(gdr) : 6.0;
    o.mergeCheck = flag("COSLAM_MERGE_CHECK", '1');
    o.mergeMinInNum = envi("COSLAM_MERGE_MIN_IN_NUM", 10);
    const char* mar = getenv("COSLAM_MERGE_MIN_AREA_RATIO");
    o.mergeMinAreaRatio = mar && mar[0] ? atof(mar) : 0.5;
    const char* mcd = getenv("COSLAM_MERGE_MAX_CAM_DIST");
    o.mergeMaxCamDist = mcd && mcd[0] ? atof(mcd) : 6.0;
    if (o.mergeCheck && !o.grouping) {
        fprintf(stderr, "COSLAM_MERGE_CHECK=1 needs COSLAM_CAMERA_GROUPING=1: the check reads the key frame's record of the groups\n");
        exit(2);
    }
    o.liveView = flag("COSLAM_LIVE_VIEW", '1');
    o.liveEvery = std::max(1, envi("COSLAM_LIVE_VIEW_EVERY", 1));
    o.liveDepth = std::max(2, envi("COSLAM_LIVE_VIEW_DEPTH", 8));
    o.liveTrailDepth = std::max(1, envi("COSLAM_LIVE_VIEW_TRAIL_DEPTH", 150));   // (150: the display's m_nTrjLen, src/gui/GLScenePane.h:26)
    o.liveCurCap = std::max(0, envi("COSLAM_LIVE_VIEW_CUR_CAP", 0));
    o.liveDynCap = std::max(0, envi("COSLAM_LIVE_VIEW_DYN_CAP", 0));
    return o;
}

// ---- the workload file ----
struct Workload {
    int nCams, W, H, L, FW, FH, nFrames, nPts, P_REG, PTS, nColBlk, nRowBlk, keyEvery, camsPerLaunch;
    std::vector<int> order;
    std::vector<double> K;
    cs_klt_config cfg;
    std::vector<std::vector<uint8_t>> frames;   // [camera][frame][H][W]
    std::vector<double> mapPts;
    // projections of the visible map points in the first frame (for the slot -> map point association that stands in for the map
    // initialisation, as in bench.py associate())
    std::vector<std::vector<int>> visIdx;
    std::vector<std::vector<double>> visUV;
    std::vector<double> R0, t0, cov;   // cov: MapPoint::cov of every map point
};

// a pre-baked BA problem of the file (joint, inter-camera): both are built live on the device now, the file keeps them for its format
static int skip_ba_problem(Reader& r) {
    const int C = r.i32(), P = r.i32(), nObs = r.i32();
    r.skip<int>(4), r.skip<double>(1);   // nCamsCon, nPtsCon, maxIter, inner; maxErr
    r.skip<double>(9 * (size_t)C + 9 * (size_t)C + 3 * (size_t)C + 3 * (size_t)P), r.skip<int>((size_t)P + 1 + nObs), r.skip<double>(2 * (size_t)nObs);
    return C;
}

// the header: what check_config needs
static Workload read_header(const Options& o, Reader& rd) {
    rd.f = fopen(o.workload, "rb");
    if (!rd.f) {
        perror(o.workload);
        exit(1);
    }
    char magic[8];
    if (fread(magic, 1, 8, rd.f) != 8 || memcmp(magic, "CSWL1\0\0\0", 8) != 0) {
        fprintf(stderr, "%s is not a workload file\n", o.workload);
        exit(1);
    }
    Workload w;
    const std::vector<int> hd = rd.vec<int>(16);
    w.nCams = hd[0], w.W = hd[1], w.H = hd[2], w.L = hd[3], w.FW = hd[4], w.FH = hd[5], w.nFrames = hd[6];
    w.nPts = hd[8], w.P_REG = hd[9], w.PTS = hd[10], w.nColBlk = hd[11], w.nRowBlk = hd[12], w.keyEvery = hd[13];
    w.camsPerLaunch = o.camsPerLaunch >= 0 ? o.camsPerLaunch : hd[14];
    w.order.resize(hd[7]);
    return w;
}

// the rest of the file
static void read_body(Reader& rd, Workload& w) {
    w.order = rd.vec<int>(w.order.size());
    w.K = rd.vec<double>(9);
    const std::vector<int> ci = rd.vec<int>(6);      // nIterations, nLevels, levelSkip, windowWidth, trackWithGain, minDistance
    const std::vector<float> cf = rd.vec<float>(5);  // trackBorderMargin, convergenceThreshold, SSD_Threshold, minCornerness, detectBorderMargin
    w.cfg.nIterations = ci[0], w.cfg.nLevels = ci[1], w.cfg.levelSkip = ci[2], w.cfg.windowWidth = ci[3], w.cfg.trackWithGain = ci[4],
    w.cfg.minDistance = ci[5];
    w.cfg.trackBorderMargin = cf[0], w.cfg.convergenceThreshold = cf[1], w.cfg.SSD_Threshold = cf[2], w.cfg.minCornerness = cf[3],
    w.cfg.detectBorderMargin = cf[4];
    for (int c = 0; c < w.nCams; ++c) w.frames.push_back(rd.vec<uint8_t>((size_t)w.W * w.H * w.nFrames));
    w.mapPts = rd.vec<double>(3 * (size_t)w.nPts);
    w.visIdx.resize(w.nCams), w.visUV.resize(w.nCams);
    for (int c = 0; c < w.nCams; ++c) {
        const int nv = rd.i32();
        w.visIdx[c] = rd.vec<int>(nv);
        w.visUV[c] = rd.vec<double>(2 * (size_t)nv);
    }
    w.R0 = rd.vec<double>(9 * (size_t)w.nCams), w.t0 = rd.vec<double>(3 * (size_t)w.nCams);
    w.cov = rd.vec<double>(9 * (size_t)std::max(w.nPts, 2 * w.P_REG));
    const int jointC = skip_ba_problem(rd);
    skip_ba_problem(rd);
    // the pre-baked camera graphs (the graphs are built live now) and the ground-truth fundamental matrices [frame][pair][9] (the matching leg
    // forms F from the poses it has solved, cs_ncc_fmats_dev): read past
    const int pgGraphs = rd.i32(), pgNodesPer = rd.i32(), pgNodes = pgGraphs * pgNodesPer;
    rd.skip<uint8_t>(pgNodes), rd.skip<double>(12 * (size_t)pgNodes), rd.skip<int>(jointC);
    rd.skip<double>((size_t)w.nFrames * (w.nCams - 1) * 9);
    fclose(rd.f);
}

// the loop's argument errors that need the workload: exit 1 before any GPU work
static void check_config(const Options& o, const Workload& w) {
    if (o.world < 1 || o.rank < 0 || o.rank >= o.world || w.nCams % o.world) {
        fprintf(stderr, "%d cameras do not shard over %d ranks (rank %d)\n", w.nCams, o.world, o.rank);
        exit(1);
    }
    // a window is applied baLag * keyEvery frames behind its key frame, which the decision places kfLag frames late: with kfLag >= that the
    // apply would be due in the past and bundle adjustment silently off
    if (o.kfDrives && o.kfLag >= o.baLag * w.keyEvery) {
        fprintf(stderr, "COSLAM_KEYFRAME_LAG=%d: must be below the BA apply lag of %d x %d frames\n", o.kfLag, o.baLag, w.keyEvery);
        exit(1);
    }
}

// ---- the window schedule: window k is solved by rank k % world (the ring is identical on every rank); its packed result is broadcast and
// applied by every rank baLag key-frame intervals behind its key frame (RobustBundleRTS::output())
static const int WIN_KF = 5;   // key frames per window
struct WindowSchedule {
    struct Due {
        int frame, firstKey;
        long long seq;   // the record's sequence number ON ITS OWNER (windows go round the ranks: the owner's (k / world)-th solve)
        int k, owner;    // window number, the rank that solves it (k % world)
        std::vector<int> frames;   // the window's key frames where the decision put them (empty: firstKey + j * keyEvery)
    };
    // set up by the loop
    int rank, world, baLag, keyEvery, nCams, histStore;
    hipStream_t s;
    cs_ba* ws;
    cs_ba_window* win;
    cs_ba_output* bout;
    cs_comm* comm;
    size_t recordBytes;
    unsigned char* recv[2];   // N > 1: records solved by other ranks arrive here
    int* applyCnt;
    // the schedule
    std::vector<Due> due;      // applies still to come, in frame order
    std::vector<int> pushed;   // the frames of the key frames in the ring
    int nPushed = 0, nApplied = 0, nNotApplied = 0;
    long long nRequested = 0, nMySolves = 0;

    // behind every push into the window ring; once the ring holds WIN_KF key frames, the window that ends at frame f is requested
    // (requestForBA(5, 2, 2, 30): the numCams * 2 oldest key cameras and 2 points held, maxIter 2, inner 10; static points only)
    void request(int f, bool placed, double* dMap, const unsigned char* dMapFlags) {
        pushed.push_back(f);
        if ((int)pushed.size() > WIN_KF) pushed.erase(pushed.begin());
        if (++nPushed < WIN_KF) return;
        const int k = (int)nRequested++, owner = k % world;
        long long seq = k / world;
        if (owner == rank) {
            CSCHK(cs_ba_solve_window_flags_async(ws, win, (void*)s, dMap, dMapFlags, 2 * nCams, 2, 6.0, 2, 10));
            seq = nMySolves++;
        }
        Due d{f + baLag * keyEvery, f - (WIN_KF - 1) * keyEvery, seq, k, owner, {}};
        if (placed) d.frames = pushed, d.firstKey = pushed.front();
        due.push_back(d);
    }
    // output() of the window whose lag ends at frame i, before anything of frame i touches the map: the pose stream waits ON THE DEVICE
    // for the worker to publish the record; the host goes on enqueueing
    void apply_due(int i, cs_track_history* hist, const cs_poseupdate_cam* pu, int* dPf, int nMap, double* dMap, double* dCov,
                   unsigned char* dMapFlags, double pix, double* R, double* T) {
        if (!due.empty() && due.front().frame == i && !due.front().frames.empty() && (i - 1) - due.front().frames.front() + 1 > histStore) {
            due.erase(due.begin());   // (the camera graphs would start behind the pose history's oldest frame: the record is consumed, nothing written back)
            ++nNotApplied;
        }
        if (due.empty() || due.front().frame != i) return;
        const Due& d = due.front();
        void* rec = nullptr;
        if (d.owner == rank)
            CSCHK(cs_ba_output_wait_dev(bout, d.seq, (void*)s, 0, &rec));
        else
            rec = recv[d.k & 1];
        if (world > 1) CSCHK(cs_comm_broadcast_dev(comm, (void*)s, rec, recordBytes, d.owner));   // the owner's record to every replica
        if (!d.frames.empty())
            CSCHK(cs_ba_output_apply_frames_dev(bout, rec, d.seq, (void*)s, hist, win, pu, dPf, nMap, dMap, dCov, dMapFlags, pix, d.frames.data(),
                                                (int)d.frames.size(), R, T, applyCnt));
        else
            CSCHK(cs_ba_output_apply_seq_dev(bout, rec, d.seq, (void*)s, hist, win, pu, dPf, nMap, dMap, dCov, dMapFlags, pix, d.firstKey, keyEvery,
                                             R, T, applyCnt));
        due.erase(due.begin());
        ++nApplied;
    }
};

// ---- the key-frame decision (COSLAM_KEYFRAME_DRIVES=1): the key frames where CoSLAM::genNewMapPoints' decision puts them
// (src/app/SL_CoSLAM.cpp:1294-1346: one camera's mapped points decreased -> addKeyFrame for all cameras -> requestForBA) instead of the
// fixed cadence -- and no host wait per frame: the decision word of frame i goes into pinned memory behind an event, the host acts on the
// decision of frame i - COSLAM_KEYFRAME_LAG (>= 1), the key frame's own records and poses come out of a ring of LAG + 1 snapshots
// (coslam_amd/frameloop.py: LoopConfig.keyframe_lag)
struct KfSnap {
    double *xy, *R, *t;
    int *st, *s2m, *word;   // word: pinned host memory
    hipEvent_t ev;
    int frame;
    std::vector<cs_handback_cam> hb;
};

// ---- the loop: device state, set-up and per-frame stages ----
struct FrameLoop {
    const Options& o;
    const Workload& w;
    int nCams, W, H, N, nc, c0, nMap, keyEvery, P_REG, PTS;
    size_t imgBytes;
    // Const::PIXEL_ERR_VAR = 10 (reference src/app/SL_GlobParam.cpp:37) is a VARIANCE (the retired define beside it: `SLAM_PIXEL_ERR_VAR 4
    // //2 pixels error`, src/slam/SL_Define.h:16); this library's getProjectionCovMat / seqTriangulate / getTriangulateCovMat take a standard
    // deviation: sqrt(10) px.  COSLAM_PIXEL_ERR_STD=1: the constant handed over as it is (a 10 px gate: rounds 1-4).  DESIGN.md 5.1
    static constexpr double PIXVAR = 10.0;
    double PIX, PIX_CLASSIFY;
    // the map keeps spare capacity behind the scene's points: NewMapPtsNCC's new points are appended (cs_newpts_from_pairs_dev)
    static const int MAP_SPARE = 8192;
    static const int RV_CAP = 1024, RV_ROUNDS = 2;   // the second visits' rounds (cs_register_revisit_*)
    static const int NCC_EVERY = 4;
    static const int NCC_PAIR_CAP = 1 << 16;   // passing pairs kept per camera pair and run (cs_ncc_epi_pairs_dev)

    // tracking
    hipStream_t kltS, poseS;
    std::vector<cs_klt*> trk;   // the rank's own cameras: c0 + k
    cs_klt_group* grp;
    std::vector<uint8_t*> dFrames;
    cs_klt_feature* dDest[2][16];
    int* dCnt[16];
    hipEvent_t kltDone[2], destFree[2];
    // the map and the frame's records
    double *dK, *dKall, *dKud, *dMap, *dCov, *diK, *dXY, *dMs, *dms, *dReproj;
    int *dMapCount, *dS2M, *dSpan, *dState, *dSel, *dNpts, *dOk, *dPf, *dSfn, *dFirstFrm;
    cs_pose_option* dOpt;
    unsigned char *dIsStatic, *dMapFlags, *dMergeable, *dNewPt;
    double* dR[2];
    double* dT[2];
    cs_track_history* hist;
    std::vector<cs_handback_cam> hb[2];   // all cameras (the window's push reads xy / state / slot2map)
    std::vector<cs_handback_cam> hbOwn[2], hbOther;   // the rank's own cameras from their trackers' dest[]; the others from the gathered records
    std::vector<cs_register_cam> rc[2];
    std::vector<cs_poseupdate_cam> pu;
    std::vector<int*> s2mPtrs;
    // N > 1: the communicator, the per-frame exchange of {dest[], R, t}, the candidates' all-gather
    cs_comm* comm = nullptr;
    cs_exchange* xchg = nullptr;
    unsigned char* xRecv = nullptr;
    size_t xRecBytes = 0;
    int *dCandSend = nullptr, *dCandRecv = nullptr;
    // registration
    void* dMergeCache;
    cs_feat_ref* dFref;
    unsigned char* dRstat;
    int *dFrefCnt, *dCurList, *dCurCount, *dCurOverflow;
    int *dRvList, *dRvVisit, *dRvNext, *dRvCnt, *dRvListCnt, *dRvLists, *dRvCounts;
    unsigned char* dRvReg[2];   // current points beyond the list's cap P_REG (left out of that frame's registration)
    int* dMergeRun;
    struct RegOut {
        int *slot, *flags;
        double *m, *var, *dist;
    } reg;
    unsigned char *dAttached, *dRegged;
    void *dDecScratch, *dMergeScratch;
    int *dDecCnt, *dMergeCnt;
    int nMergeFrames = 0;
    // key-frame solves
    cs_ba *jointWs, *icWs;
    cs_ba_window* win;
    cs_ba_intercam* icam;
    std::vector<cs_intercam_cam> icCams;
    cs_ba_output* bout;
    WindowSchedule sched;
    int nKey = 0;
    // the key-frame decision's state (cs_keyframe_ready_dev)
    int *dKfFrame, *dKfMapped, *dKfReady, *dKfCnt, *dKfStats;
    double *dKfSelfR, *dKfSelfT, *dKfCen;
    double kfMinTranslation = 0.1;
    std::vector<cs_keyframe_cam> kfCams[2];
    std::vector<KfSnap> kfRing;
    std::vector<int> kfPlaced;
    // inter-camera NCC matching every 4th frame
    unsigned char *dSmall, *dBlk;
    double *dAbc, *dFm;
    int *dValid, *dPairCount, *dNpCounts;
    cs_ncc_pair* dPairs;
    void* dNpScratch;
    std::vector<cs_ncc_cam> ncams;
    std::vector<cs_ncc_pair_job> jobs;
    std::vector<const cs_ncc_pair*> pairPtr;
    std::vector<const int*> cntPtr;
    std::vector<int> pairA, pairB;
    std::vector<const double*> pairIK;
    int nccRuns = 0;
    // CoSLAM::cameraGrouping per frame (COSLAM_CAMERA_GROUPING=1), reported only: a device ring of results, its older half read by the host
    // when the newer one has been filled since (behind an event that is half a ring old: never a wait for the frame in flight)
    static constexpr int GROUP_RING = 128;
    double grpInitTranslation = 0.0;   // m_initCamTranslation (src/app/SL_CoSLAM.cpp:280-290)
    std::vector<cs_grouping_cam> grpCams[2];
    cs_camera_groups* dGrpGroups = nullptr;
    double* dGrpCosts = nullptr;
    int* dGrpShare = nullptr;
    void* dGrpScratch = nullptr;
    hipEvent_t grpEv[2];
    hipStream_t grpCopyS = nullptr;
    long long grpCalls = 0, grpTaken = 0;
    std::vector<int> grpPerFrame;
    int grpMoreThanOne = 0, grpFirstSuch = -1, grpChanges = 0;
    bool grpHaveLast = false;
    cs_camera_groups grpLast;
    std::vector<double> grpLastCosts;
    // MergeCameraGroup::checkPossibleMergable at every key frame (COSLAM_MERGE_CHECK=1), reported only: a device ring of records
    // (KeyFrame::setCamGroups plus the check's result), read by the host as the grouping's ring is
    static constexpr int MERGE_RING = 32;
    cs_merge_candidates* dMrgRing = nullptr;
    void* dMrgScratch = nullptr;
    hipEvent_t mrgEv[2];
    long long mrgCalls = 0, mrgTaken = 0;
    std::vector<int> mrgFrames;
    int mrgSplit = 0, mrgWithCandidate = 0, mrgFirstSuch = -1;
    bool mrgHaveLast = false;
    cs_merge_candidates mrgLast;
    // the frame's last step (COSLAM_LIVE_VIEW=1): storeDynamicPoints + the display's copy, one launch per frame on the pose stream, no wait
    cs_liveview* live = nullptr;
    int liveFrames = 0, livePublished = 0;
    // drain
    int* dBar;
    int nEmptySolves = 0;
    int nDone = 0;

    FrameLoop(const Options& opt, const Workload& wl) : o(opt), w(wl) {
        nCams = w.nCams, W = w.W, H = w.H, N = w.FW * w.FH, nc = nCams / o.world, c0 = o.rank * nc, nMap = w.nPts + MAP_SPARE;
        keyEvery = w.keyEvery, P_REG = w.P_REG, PTS = w.PTS, imgBytes = (size_t)W * H;
        PIX = o.pixIsStd ? PIXVAR : sqrt(PIXVAR), PIX_CLASSIFY = o.pixIsStd ? 12.0 : sqrt(12.0);
    }

    void setup_trackers(std::vector<std::vector<uint8_t>>& frames);
    void setup_state();
    void setup_comm();
    void setup_registration();
    void setup_keyframe_solves();
    void setup_keyframe_decision();
    void setup_ncc();
    void setup_cameras();
    void setup_window_records();
    void setup_decision_scratch();
    void first_frame();
    void associate();
    void step(int i, bool key);
    void ncc_leg(int i, int f, int dsti);
    void register_frame(int i, int dsti);
    void key_frame_actions(int f, const cs_handback_cam* cams, const double* Rk, const double* tk, bool placed, int dsti);
    void keyframe_decision_step(int i, int dsti);
    void setup_camera_grouping();
    void camera_grouping(int i, int dsti);
    void grouping_take(int n, bool synced);
    std::string grouping_json();
    void setup_merge_check();
    void merge_check(int f, const cs_handback_cam* cams, const double* Rk, const double* tk);
    void merge_take(int n, bool synced);
    std::string merge_json();
    void live_view(int i, int dsti);
    std::string live_json();
    void run(int n) {
        for (int q = 0; q < n; ++q, ++nDone) step(nDone + 1, keyEvery > 0 && nDone % keyEvery == 0);
    }
    void wait_ws(cs_ba* ws);
    void barrier();
    void report(double dt, double dtHost, int applied0, const int rvCnt0[4]);
    void export_results();
};

// frames resident in HBM before the clock starts, like bench.py's headline; the trackers of the rank's own cameras as one group
void FrameLoop::setup_trackers(std::vector<std::vector<uint8_t>>& frames) {
    dFrames.resize(nCams);
    for (int c = 0; c < nCams; ++c) {
        dFrames[c] = to_dev(frames[c]);
        std::vector<uint8_t>().swap(frames[c]);
    }
    HIPCHK(hipStreamCreateWithFlags(&kltS, hipStreamNonBlocking));
    HIPCHK(hipStreamCreateWithFlags(&poseS, hipStreamNonBlocking));
    trk.resize(nc);
    for (int c = 0; c < nc; ++c) {
        trk[c] = made(cs_klt_create(&w.cfg, o.dev, 0), "cs_klt_create");
        CSCHK(cs_klt_allocate(trk[c], W, H, w.L, w.FW, w.FH, 0, 0));
        if (!o.kltFused) CSCHK(cs_klt_set_fused(trk[c], 0));
    }
    grp = made(cs_klt_group_create(trk.data(), nc), "cs_klt_group_create");
    CSCHK(cs_klt_group_set_stream(grp, (void*)kltS));
    if (w.camsPerLaunch > 0)  // the co-residency budget of `camsPerLaunch` cameras (250 waves each, 8 resident waves per CU)
        for (cs_klt* k : trk) CSCHK(cs_klt_set_cu_count(k, std::min(256, (250 * w.camsPerLaunch + 60) / 8 + 5)));
}

// the map, the frame's records and the camera descriptors over them
void FrameLoop::setup_state() {
    const std::vector<double>& K = w.K;
    dK = to_dev(K);
    std::vector<double> Kall;
    for (int c = 0; c < nCams; ++c) Kall.insert(Kall.end(), K.begin(), K.end());
    dKall = to_dev(Kall);
    dKud = dev_zeros<double>(7);
    dMap = dev_zeros<double>(3 * (size_t)nMap);
    dCov = dev_zeros<double>(9 * (size_t)std::max(nMap, 2 * P_REG));
    HIPCHK(hipMemcpy(dMap, w.mapPts.data(), sizeof(double) * w.mapPts.size(), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(dCov, w.cov.data(), sizeof(double) * w.cov.size(), hipMemcpyHostToDevice));
    dMapCount = dev_zeros<int>(1);
    HIPCHK(hipMemcpy(dMapCount, &w.nPts, sizeof(int), hipMemcpyHostToDevice));
    dS2M = dev_zeros<int>((size_t)nCams * N);
    dSpan = dev_zeros<int>((size_t)nCams * 2 * N);
    HIPCHK(hipMemset(dS2M, 0xff, sizeof(int) * (size_t)nCams * N));
    HIPCHK(hipMemset(dSpan, 0xff, sizeof(int) * (size_t)nCams * 2 * N));
    dXY = dev_zeros<double>((size_t)nCams * 2 * N);
    dState = dev_zeros<int>((size_t)nCams * N);
    dMs = dev_zeros<double>((size_t)nCams * PTS * 3);
    dms = dev_zeros<double>((size_t)nCams * PTS * 2);
    dSel = dev_zeros<int>((size_t)nCams * PTS);
    dNpts = dev_zeros<int>(nCams);
    dOpt = (cs_pose_option*)dev_zeros<unsigned char>((size_t)nCams * sizeof(cs_pose_option));
    dOk = dev_zeros<int>(nCams);
    dPf = dev_zeros<int>((size_t)nMap * nCams);  // MapPoint::pFeatures of this frame, nMap x nCams (the hand-back writes it)
    HIPCHK(hipMemset(dPf, 0xff, sizeof(int) * (size_t)nMap * nCams));
    // poseUpdate3D's second half + detectDynamicFeaturePoints behind the pose solve (cs_pose_update_frame_dev)
    const std::vector<double> iKh = {1 / K[0], -K[1] / (K[0] * K[4]), (K[1] * K[5] - K[2] * K[4]) / (K[0] * K[4]), 0, 1 / K[4], -K[5] / K[4], 0, 0, 1};
    diK = to_dev(iKh);
    dFm = dev_zeros<double>((size_t)16 * 9);   // the camera pairs' fundamental matrices of a matching run
    dIsStatic = dev_zeros<unsigned char>((size_t)nCams * N);
    HIPCHK(hipMemset(dIsStatic, 1, (size_t)nCams * N));
    dReproj = dev_zeros<double>((size_t)nCams * N);
    dMapFlags = dev_zeros<unsigned char>(nMap);
    dMergeable = dev_zeros<unsigned char>((size_t)nMap * nCams);   // the registration's tables are indexed by the MAP index
    // CoSLAM::mapPointsClassify behind the pose update: MapPoint::bNewPt / staticFrameNum / firstFrame of every map point
    dNewPt = dev_zeros<unsigned char>(nMap);
    dSfn = dev_zeros<int>(nMap);
    dFirstFrm = dev_zeros<int>(nMap);
    // walks 64 frames deep; 4096 frames (COSLAM_HIST_STORE) of pixels + poses kept behind them for the running whole-track mergability verdict
    hist = made(cs_track_history_create_ex(o.dev, nCams, N, 64, o.histStore), "cs_track_history_create_ex");
    if (o.exportFrames > 0) CSCHK(cs_track_history_set_archive(hist, o.exportFrames));   // every frame that leaves the store kept, for the export
}

// N > 1: rank r owns cameras r * nc .. r * nc + nc - 1: their images, trackers, hand-backs and pose solves; everything behind the per-frame
// all-gather of {dest[], R, t} is replayed on every rank's own replica of the map.  The communicator: RCCL through the
// library's own cs_comm_*, or the test transport for ranks sharing one GPU
void FrameLoop::setup_comm() {
    if (o.hostSegment) {
        comm = cs_comm_create_host(o.hostSegment, o.world, o.rank, o.dev);
    } else {
        // rank 0 creates the unique id and leaves it in COSLAM_COMM_ID_FILE (written to a temporary name, then renamed); the others poll
        const char* path = o.commIdFile;
        unsigned char id[128];
        if (!path || !cs_comm_available()) {
            fprintf(stderr, "N > 1 needs COSLAM_COMM_ID_FILE (or COSLAM_COMM=host:<name>) and RCCL: %s\n", cs_last_error());
            exit(3);
        }
        if (o.rank == 0) {
            CSCHK(cs_comm_unique_id(id));
            const std::string tmp = std::string(path) + ".tmp";
            FILE* f = fopen(tmp.c_str(), "wb");
            if (!f || fwrite(id, 1, 128, f) != 128 || fclose(f) != 0 || rename(tmp.c_str(), path) != 0) {
                perror(path);
                exit(3);
            }
        } else {
            bool got = false;
            for (int tries = 0; tries < 12000 && !got; ++tries) {   // up to 60 s
                FILE* f = fopen(path, "rb");
                if (f) {
                    got = fread(id, 1, 128, f) == 128;
                    fclose(f);
                }
                if (!got) std::this_thread::sleep_for(std::chrono::milliseconds(5));
            }
            if (!got) {
                fprintf(stderr, "rank %d: no unique id in %s after 60 s\n", o.rank, path);
                exit(3);
            }
        }
        comm = cs_comm_create(id, o.world, o.rank, o.dev);
    }
    if (!comm || !(xchg = cs_exchange_create(comm, nc, N))) {
        fprintf(stderr, "rank %d: communicator: %s\n", o.rank, cs_last_error());
        exit(3);
    }
    void* rv = nullptr;
    CSCHK(cs_exchange_buffers(xchg, &rv, &xRecBytes));
    xRecv = (unsigned char*)rv;
    dCandSend = dev_zeros<int>((size_t)3 * nc * P_REG);
    dCandRecv = dev_zeros<int>((size_t)3 * nc * P_REG * o.world);
}

void FrameLoop::setup_registration() {
    dMergeCache = dev_zeros<unsigned char>(cs_register_mergability_cache_bytes(nMap, nCams));
    // MapPoint::pFeatures as feature references (stale features are views, re-linked chains: SL_CoSLAM.cpp:775-779)
    dFrefCnt = dev_zeros<int>(5);
    HIPCHK(hipMalloc((void**)&dFref, sizeof(cs_feat_ref) * (size_t)nMap * nCams));
    HIPCHK(hipMemset(dFref, 0xff, sizeof(cs_feat_ref) * (size_t)nMap * nCams));   // (-1 everywhere: no feature)
    dRstat = dev_zeros<unsigned char>((size_t)nMap * nCams);
    dCurList = dev_zeros<int>(nMap);
    dCurCount = dev_zeros<int>(1);
    dCurOverflow = dev_zeros<int>(1);
    dRvList = dev_zeros<int>(RV_CAP);
    dRvVisit = dev_zeros<int>(nMap), dRvNext = dev_zeros<int>(nMap), dRvCnt = dev_zeros<int>(4), dRvListCnt = dev_zeros<int>(4);
    dRvLists = dev_zeros<int>((size_t)RV_ROUNDS * RV_CAP), dRvCounts = dev_zeros<int>(RV_ROUNDS + 1);
    dRvReg[0] = dev_zeros<unsigned char>(nMap), dRvReg[1] = dev_zeros<unsigned char>(nMap);
    dMergeRun = dev_zeros<int>(4);
    dR[0] = to_dev(w.R0), dR[1] = to_dev(w.R0);
    dT[0] = to_dev(w.t0), dT[1] = to_dev(w.t0);
    for (int c = 0; c < nCams; ++c) {
        dDest[0][c] = dev_zeros<cs_klt_feature>(N);
        dDest[1][c] = dev_zeros<cs_klt_feature>(N);
        dCnt[c] = dev_zeros<int>(4);
    }
    reg.slot = dev_zeros<int>((size_t)nMap * nCams), reg.flags = dev_zeros<int>((size_t)nMap * nCams);
    reg.m = dev_zeros<double>((size_t)nMap * nCams * 2), reg.var = dev_zeros<double>((size_t)nMap * nCams * 4);
    reg.dist = dev_zeros<double>((size_t)nMap * nCams);
    HIPCHK(hipMemset(reg.slot, 0xff, sizeof(int) * (size_t)nMap * nCams));
}

// key-frame solves: the joint local BA parsed on the device from the ring of the last 5 key frames (cs_ba_window_*: the hand-back's records
// and the poses of every camera at the key frame), like bench.py's N = 1 default; the inter-camera problem built on the device from every key
// frame's records (InterCamPoseEstimator::addMapPoints); RobustBundleRTS::output(): every window solve's result packed by the worker
void FrameLoop::setup_keyframe_solves() {
    jointWs = cs_ba_create(o.dev);
    win = cs_ba_window_create(o.dev, nCams, WIN_KF, N, nMap);
    if (!jointWs || !win) made<void>(nullptr, "cs_ba_window_create");
    CSCHK(cs_ba_reserve_for_window(jointWs, win));  // (the result buffers' addresses are final from here on)
    icWs = cs_ba_create(o.dev);
    icam = cs_ba_intercam_create(o.dev, nCams, N, PTS, nMap, 60);
    if (!icWs || !icam) made<void>(nullptr, "cs_ba_intercam_create");
    icCams.resize(nCams);
    for (int c = 0; c < nCams; ++c) {
        icCams[c].K = dK, icCams[c].xy = dXY + (size_t)c * 2 * N, icCams[c].state = dState + (size_t)c * N;
        icCams[c].slot2map = dS2M + (size_t)c * N, icCams[c].trackSpan = dSpan + (size_t)c * 2 * N, icCams[c].isStatic = dIsStatic + (size_t)c * N;
    }
    bout = made(cs_ba_output_create(o.dev, nCams, WIN_KF, nMap, o.kfDrives ? std::min(o.baLag * keyEvery + 6, 64) : 8), "cs_ba_output_create");
    CSCHK(cs_ba_output_attach(bout, jointWs));
    CSCHK(cs_ba_output_set_feat_refs(bout, dFref, dRstat));
    CSCHK(cs_track_history_set_classify_refs(hist, dFref, dRstat));   // mapPointsClassify over the references
    CSCHK(cs_track_history_set_merge_refs(hist, dFref, dRstat));      // ... and the bMerge walks
    WindowSchedule& s = sched;
    s.rank = o.rank, s.world = o.world, s.baLag = o.baLag, s.keyEvery = keyEvery, s.nCams = nCams, s.histStore = o.histStore, s.s = poseS;
    s.ws = jointWs, s.win = win, s.bout = bout, s.comm = comm, s.recordBytes = cs_ba_output_record_bytes(bout);
}

// the key-frame decision's state (cs_keyframe_ready_dev) as CoSLAM::initMap leaves it: a key pose with self motion in every camera at frame
// 0, nMappedPts 0, m_minCamTranslation = the mean distance between the cameras / 4.5 (src/app/SL_CoSLAM.cpp:246-256, :278-291)
void FrameLoop::setup_keyframe_decision() {
    dKfFrame = dev_zeros<int>(nCams), dKfMapped = dev_zeros<int>(nCams), dKfReady = dev_zeros<int>(nCams + 2), dKfCnt = dev_zeros<int>(2 * nCams);
    dKfStats = dev_zeros<int>(5);
    dKfSelfR = dev_zeros<double>(9 * (size_t)nCams), dKfSelfT = dev_zeros<double>(3 * (size_t)nCams), dKfCen = dev_zeros<double>(3 * (size_t)nCams);
    if (!o.kfDrives) return;
    HIPCHK(hipMemcpy(dKfSelfR, dR[0], sizeof(double) * 9 * nCams, hipMemcpyDeviceToDevice));
    HIPCHK(hipMemcpy(dKfSelfT, dT[0], sizeof(double) * 3 * nCams, hipMemcpyDeviceToDevice));
    std::vector<double> hR(9 * (size_t)nCams), hT(3 * (size_t)nCams), cen(3 * (size_t)nCams);
    HIPCHK(hipMemcpy(hR.data(), dR[0], sizeof(double) * hR.size(), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(hT.data(), dT[0], sizeof(double) * hT.size(), hipMemcpyDeviceToHost));
    for (int c = 0; c < nCams; ++c)
        for (int k = 0; k < 3; ++k) cen[3 * c + k] = -(hR[9 * c + k] * hT[3 * c] + hR[9 * c + 3 + k] * hT[3 * c + 1] + hR[9 * c + 6 + k] * hT[3 * c + 2]);
    double sum = 0;
    int n = 0;
    for (int a = 0; a < nCams; ++a)
        for (int c = a + 1; c < nCams; ++c, ++n) {
            const double d0 = cen[3 * a] - cen[3 * c], d1 = cen[3 * a + 1] - cen[3 * c + 1], d2 = cen[3 * a + 2] - cen[3 * c + 2];
            sum += sqrt(d0 * d0 + d1 * d1 + d2 * d2);
        }
    if (n > 0) kfMinTranslation = sum / n / 4.5;
    for (int q = 0; q < 2; ++q) {
        kfCams[q].resize(nCams);
        for (int c = 0; c < nCams; ++c) {
            cs_keyframe_cam& k = kfCams[q][c];
            k.state = dState + (size_t)c * N, k.slot2map = dS2M + (size_t)c * N, k.R = dR[q] + 9 * c, k.t = dT[q] + 3 * c;
            k.keyFrame = dKfFrame + c, k.keyMapped = dKfMapped + c, k.selfR = dKfSelfR + 9 * c, k.selfT = dKfSelfT + 3 * c;
        }
    }
    kfRing.resize(o.kfLag + 1);
    for (KfSnap& sn : kfRing) {
        sn.xy = dev_zeros<double>((size_t)nCams * 2 * N), sn.R = dev_zeros<double>(9 * (size_t)nCams), sn.t = dev_zeros<double>(3 * (size_t)nCams);
        sn.st = dev_zeros<int>((size_t)nCams * N), sn.s2m = dev_zeros<int>((size_t)nCams * N);
        HIPCHK(hipHostMalloc((void**)&sn.word, sizeof(int), hipHostMallocDefault));
        *sn.word = 0;
        HIPCHK(hipEventCreateWithFlags(&sn.ev, hipEventDisableTiming));
        sn.frame = -1;
        sn.hb = hb[0];
        for (int c = 0; c < nCams; ++c)
            sn.hb[c].xy = sn.xy + (size_t)c * 2 * N, sn.hb[c].state = sn.st + (size_t)c * N, sn.hb[c].slot2map = sn.s2m + (size_t)c * N;
    }
}

// inter-camera NCC matching every 4th frame: getNCCBlocks per camera on the full frame, the matrices per consecutive pair; the descriptors
// are fixed but for the frame's images
void FrameLoop::setup_ncc() {
    int wsS = 0, hsS = 0;
    CSCHK(cs_ncc_scaled_dims(W, H, 0.3, &wsS, &hsS));
    dSmall = dev_zeros<unsigned char>((size_t)nCams * wsS * hsS);
    dBlk = dev_zeros<unsigned char>((size_t)nCams * N * 128);
    dAbc = dev_zeros<double>((size_t)nCams * N * 4);
    dValid = dev_zeros<int>((size_t)nCams * N);
    dPairs = (cs_ncc_pair*)dev_zeros<unsigned char>((size_t)(nCams > 1 ? nCams - 1 : 1) * NCC_PAIR_CAP * sizeof(cs_ncc_pair));
    dPairCount = dev_zeros<int>(nCams);
    dNpScratch = dev_zeros<unsigned char>(cs_newpts_scratch_bytes(nCams, N));
    dNpCounts = dev_zeros<int>(4 + nCams);
    if (nCams < 2) return;
    ncams.resize(nCams);
    for (int c = 0; c < nCams; ++c) {
        ncams[c].img = nullptr, ncams[c].x = dXY + (size_t)c * 2 * N, ncams[c].y = dXY + (size_t)c * 2 * N + N;
        ncams[c].scaled = dSmall + (size_t)c * wsS * hsS, ncams[c].blocks = dBlk + (size_t)c * N * 128, ncams[c].abc = dAbc + (size_t)c * N * 4;
        ncams[c].valid = dValid + (size_t)c * N;
    }
    jobs.resize(nCams - 1), pairPtr.resize(nCams - 1), cntPtr.resize(nCams - 1), pairA.resize(nCams - 1), pairB.resize(nCams - 1);
    pairIK.assign(nCams, diK);
    for (int c = 0; c + 1 < nCams; ++c) {
        memset(&jobs[c], 0, sizeof(jobs[c]));
        jobs[c].dF = dFm + 9 * (size_t)c;   // E and F from the poses this frame has solved (matchBetween, SL_NewMapPointsInterCam.cpp:284-292)
        jobs[c].camA = c, jobs[c].camB = c + 1, jobs[c].pairs = dPairs + (size_t)c * NCC_PAIR_CAP, jobs[c].count = dPairCount + c;
        pairPtr[c] = jobs[c].pairs, cntPtr[c] = jobs[c].count, pairA[c] = c, pairB[c] = c + 1;
    }
}

// the camera descriptors over the frame's records: hand-back, registration, pose update
void FrameLoop::setup_cameras() {
    for (int b = 0; b < 2; ++b) {
        hb[b].resize(nCams);
        rc[b].resize(nCams);
        for (int c = 0; c < nCams; ++c) {
            cs_handback_cam& h = hb[b][c];
            memset(&h, 0, sizeof(h));
            h.dest = dDest[b][c], h.K = dK, h.kud = dKud, h.mapPts = dMap, h.slot2map = dS2M + (size_t)c * N;
            h.trackSpan = dSpan + (size_t)c * 2 * N, h.xy = dXY + (size_t)c * 2 * N, h.state = dState + (size_t)c * N;
            h.Ms = dMs + (size_t)c * PTS * 3, h.ms = dms + (size_t)c * PTS * 2, h.sel = dSel + (size_t)c * PTS;
            h.npts = dNpts + c, h.opt = dOpt + c, h.pointFeat = dPf + c, h.pointFeatStride = nCams, h.nPointFeat = nMap;
            h.isStatic = dIsStatic + (size_t)c * N;
            cs_register_cam& r = rc[b][c];
            memset(&r, 0, sizeof(r));
            r.K = dK, r.R = dR[b] + 9 * c, r.t = dT[b] + 3 * c, r.xy = dXY + (size_t)c * 2 * N;
            r.state = dState + (size_t)c * N, r.slot2map = dS2M + (size_t)c * N;
            r.isStatic = dIsStatic + (size_t)c * N;   // (FeaturePoint::type as the pose update keeps it: a static point's walk passes DYNAMIC features by)
        }
        hbOwn[b].assign(hb[b].begin() + c0, hb[b].begin() + c0 + nc);
    }
    pu.resize(nCams);
    for (int c = 0; c < nCams; ++c) {
        memset(&pu[c], 0, sizeof(pu[c]));
        pu[c].K = dK, pu[c].iK = diK, pu[c].xy = dXY + (size_t)c * 2 * N, pu[c].state = dState + (size_t)c * N;
        pu[c].slot2map = dS2M + (size_t)c * N, pu[c].trackSpan = dSpan + (size_t)c * 2 * N;
        pu[c].reprojErr = dReproj + (size_t)c * N, pu[c].isStatic = dIsStatic + (size_t)c * N;
    }
    for (int c = 0; c < nCams; ++c) s2mPtrs.push_back(dS2M + (size_t)c * N);
    for (int c = 0; c < nCams && o.world > 1; ++c)
        if (c < c0 || c >= c0 + nc) {
            cs_handback_cam h = hb[0][c];
            h.dest = (const cs_klt_feature*)(xRecv + (size_t)c * xRecBytes);
            hbOther.push_back(h);
        }
}

// the records that an apply reads: N > 1, the ones other ranks solved arrive here
void FrameLoop::setup_window_records() {
    for (int q = 0; q < 2; ++q) sched.recv[q] = o.world > 1 ? dev_zeros<unsigned char>(sched.recordBytes) : nullptr;
    sched.applyCnt = dev_zeros<int>(3);
}

// the registration decisions' scratch
void FrameLoop::setup_decision_scratch() {
    dAttached = dev_zeros<unsigned char>((size_t)nMap * nCams);
    dRegged = dev_zeros<unsigned char>(nMap);
    dDecScratch = dev_zeros<unsigned char>(cs_register_decide_scratch_bytes(nCams, N, nMap));
    dMergeScratch = dev_zeros<unsigned char>(cs_register_decide_merge_scratch_bytes(nMap, P_REG, nCams));
    dDecCnt = dev_zeros<int>(4);
    dMergeCnt = dev_zeros<int>(4);
}

// m_initCamTranslation from the initial poses of ALL cameras (the mean pairwise distance of their centres, on the host) and the device ring
void FrameLoop::setup_camera_grouping() {
    double sum = 0.0;
    int n = 0;
    auto centre = [&](int c, double C[3]) {
        const double *R = w.R0.data() + 9 * c, *t = w.t0.data() + 3 * c;
        for (int k = 0; k < 3; ++k) C[k] = -((R[k] * t[0] + R[3 + k] * t[1]) + R[6 + k] * t[2]);
    };
    for (int a = 0; a < nCams; ++a)
        for (int b = a + 1; b < nCams; ++b, ++n) {
            double A[3], B[3];
            centre(a, A), centre(b, B);
            sum += std::sqrt((A[0] - B[0]) * (A[0] - B[0]) + (A[1] - B[1]) * (A[1] - B[1]) + (A[2] - B[2]) * (A[2] - B[2]));
        }
    grpInitTranslation = n ? sum / n : 0.0;
    for (int q = 0; q < 2; ++q) {
        grpCams[q].resize(nCams);
        for (int c = 0; c < nCams; ++c) grpCams[q][c] = cs_grouping_cam{dXY + (size_t)c * 2 * N, dR[q] + 9 * c, dT[q] + 3 * c};
    }
    dGrpGroups = dev_zeros<cs_camera_groups>(GROUP_RING);
    dGrpCosts = dev_zeros<double>((size_t)GROUP_RING * nCams * nCams);
    dGrpShare = dev_zeros<int>((size_t)GROUP_RING * nCams * nCams);
    dGrpScratch = dev_zeros<unsigned char>(cs_camera_grouping_scratch_bytes(nCams, N));   // (zeroed once: every call leaves it zeroed)
    for (int h = 0; h < 2; ++h) HIPCHK(hipEventCreateWithFlags(&grpEv[h], hipEventDisableTiming));
    HIPCHK(hipStreamCreateWithFlags(&grpCopyS, hipStreamNonBlocking));
    grpLastCosts.assign((size_t)nCams * nCams, 0.0);
}

// CoSLAM::cameraGrouping of frame i where the reference has it (src/gui/CoSLAMThread.cpp:107-109): this frame's pointFeat, pixels and map
// flags, the poses just written; rows 0 .. map count (the frame's current-points list is built later, by the registration).  One launch
void FrameLoop::camera_grouping(int i, int dsti) {
    (void)i;
    const int half = GROUP_RING / 2;
    if (grpCalls - grpTaken >= GROUP_RING) grouping_take(half, false);
    const int slot = (int)(grpCalls % GROUP_RING);
    CSCHK(cs_camera_grouping_dev(o.dev, (void*)poseS, nCams, grpCams[dsti].data(), N, nMap, dMapCount, dPf, dMapFlags, nullptr, nullptr, W, H,
                                 o.groupMinNum, o.groupMinAreaRatio, dGrpCosts + (size_t)slot * nCams * nCams, dGrpShare + (size_t)slot * nCams * nCams,
                                 nullptr, dGrpScratch, grpInitTranslation, o.groupMaxDistRatio, dGrpGroups + slot));
    if (++grpCalls % half == 0) HIPCHK(hipEventRecord(grpEv[(slot / half) & 1], poseS));
}

// the oldest n results of the ring to the host: one copy of the records and one of the costs per stretch of the ring, one wait
void FrameLoop::grouping_take(int n, bool synced) {
    const int half = GROUP_RING / 2;
    const size_t nn = (size_t)nCams * nCams;
    std::vector<cs_camera_groups> g;
    std::vector<double> costs;
    for (int k = 0; k < n;) {
        const int slot = (int)((grpTaken + k) % GROUP_RING), seg = std::min(n - k, GROUP_RING - slot);
        if (!synced && k == 0) HIPCHK(hipEventSynchronize(grpEv[(slot / half) & 1]));
        g.resize(seg), costs.resize(seg * nn);
        HIPCHK(hipMemcpyAsync(g.data(), dGrpGroups + slot, sizeof(cs_camera_groups) * seg, hipMemcpyDeviceToHost, grpCopyS));
        HIPCHK(hipMemcpyAsync(costs.data(), dGrpCosts + (size_t)slot * nn, sizeof(double) * seg * nn, hipMemcpyDeviceToHost, grpCopyS));
        HIPCHK(hipStreamSynchronize(grpCopyS));
        for (int q = 0; q < seg; ++q) {
            if (g[q].groupNum > 1) {
                ++grpMoreThanOne;
                if (grpFirstSuch < 0) grpFirstSuch = (int)(grpTaken + k + q) + 1;   // (the loop's frames are 1, 2, ...: one call per frame)
            }
            if (grpHaveLast && memcmp(&grpLast, &g[q], sizeof(cs_camera_groups)) != 0) ++grpChanges;
            grpPerFrame.push_back(g[q].groupNum);
            grpLast = g[q], grpHaveLast = true;
        }
        std::copy(costs.end() - nn, costs.end(), grpLastCosts.begin());
        k += seg;
    }
    grpTaken += n;
}

std::string FrameLoop::grouping_json() {
    if (!o.grouping) return "null";
    grouping_take((int)(grpCalls - grpTaken), true);   // (behind the barrier)
    std::string s = "{\"groups_per_frame\": [";
    for (size_t q = 0; q < grpPerFrame.size(); ++q) s += (q ? ", " : "") + std::to_string(grpPerFrame[q]);
    s += "], \"last_groups\": [";
    if (grpHaveLast)
        for (int g = 0; g < grpLast.groupNum; ++g) {
            s += g ? ", [" : "[";
            for (int k = 0; k < grpLast.num[g]; ++k) s += (k ? ", " : "") + std::to_string(grpLast.camIds[g][k]);
            s += "]";
        }
    s += "], \"frames_with_more_than_one_group\": " + std::to_string(grpMoreThanOne) + ", \"first_such_frame\": " +
         (grpFirstSuch < 0 ? std::string("null") : std::to_string(grpFirstSuch)) + ", \"group_changes\": " + std::to_string(grpChanges) +
         ", \"last_vcosts\": [";
    for (int a = 0; a < nCams; ++a) {
        s += a ? ", [" : "[";
        for (int b = 0; b < nCams; ++b) s += (b ? ", " : "") + std::to_string((long long)grpLastCosts[(size_t)a * nCams + b]);
        s += "]";
    }
    char buf[64];
    snprintf(buf, sizeof(buf), "%.17g", grpInitTranslation);
    return s + "], \"init_cam_translation\": " + buf + "}";
}

// the device ring of the key frames' merge-check records
void FrameLoop::setup_merge_check() {
    dMrgRing = dev_zeros<cs_merge_candidates>(MERGE_RING);
    dMrgScratch = dev_zeros<unsigned char>(cs_merge_check_scratch_bytes(nCams, N));   // (zeroed once: every call leaves it zeroed)
    for (int h = 0; h < 2; ++h) HIPCHK(hipEventCreateWithFlags(&mrgEv[h], hipEventDisableTiming));
}

// checkPossibleMergable of key frame f at its push: the frame's records and poses (as they stand, or a lagged decision's snapshot), the map as
// it stands, the group record cameraGrouping wrote for frame f (one grouping call per frame: frame f's is call f).  One launch, no wait
void FrameLoop::merge_check(int f, const cs_handback_cam* cams, const double* Rk, const double* tk) {
    const int half = MERGE_RING / 2;
    if (mrgCalls - mrgTaken >= MERGE_RING) merge_take(half, false);
    if (f < 1 || f > grpCalls || grpCalls - f >= GROUP_RING) {
        fprintf(stderr, "the group record of key frame %d is no longer in the ring\n", f);
        exit(1);
    }
    const int slot = (int)(mrgCalls % MERGE_RING);
    cs_merge_cam mc[16];
    for (int c = 0; c < nCams; ++c) mc[c] = cs_merge_cam{cams[c].xy, cams[c].state, cams[c].slot2map, dK, Rk + 9 * c, tk + 3 * c};
    CSCHK(cs_merge_check_dev(o.dev, (void*)poseS, nCams, mc, N, nMap, dMapCount, dMap, dMapFlags, W, H, dGrpGroups + (int)((f - 1) % GROUP_RING), f,
                             o.mergeMinInNum, o.mergeMinAreaRatio, o.mergeMaxCamDist, 0, dMrgRing + slot, dMrgScratch));
    mrgFrames.push_back(f);
    if (++mrgCalls % half == 0) HIPCHK(hipEventRecord(mrgEv[(slot / half) & 1], poseS));
}

// the oldest n records of the ring to the host
void FrameLoop::merge_take(int n, bool synced) {
    const int half = MERGE_RING / 2;
    std::vector<cs_merge_candidates> r;
    for (int k = 0; k < n;) {
        const int slot = (int)((mrgTaken + k) % MERGE_RING), seg = std::min(n - k, MERGE_RING - slot);
        if (!synced && k == 0) HIPCHK(hipEventSynchronize(mrgEv[(slot / half) & 1]));
        r.resize(seg);
        HIPCHK(hipMemcpyAsync(r.data(), dMrgRing + slot, sizeof(cs_merge_candidates) * seg, hipMemcpyDeviceToHost, grpCopyS));
        HIPCHK(hipStreamSynchronize(grpCopyS));
        for (int q = 0; q < seg; ++q) {
            mrgSplit += r[q].groupNum > 1;
            if (r[q].nMergeInfo > 0) {
                ++mrgWithCandidate;
                if (mrgFirstSuch < 0) mrgFirstSuch = mrgFrames[k + q];
            }
            mrgLast = r[q], mrgHaveLast = true;
        }
        k += seg;
    }
    mrgFrames.erase(mrgFrames.begin(), mrgFrames.begin() + n);
    mrgTaken += n;
}

std::string FrameLoop::merge_json() {
    if (!o.mergeCheck) return "null";
    merge_take((int)(mrgCalls - mrgTaken), true);   // (behind the barrier)
    std::string s = "{\"key_frames_checked\": " + std::to_string(mrgTaken) + ", \"key_frames_with_more_than_one_group\": " + std::to_string(mrgSplit) +
                    ", \"key_frames_with_a_candidate\": " + std::to_string(mrgWithCandidate) + ", \"first_such_frame\": " +
                    (mrgFirstSuch < 0 ? std::string("null") : std::to_string(mrgFirstSuch));
    if (!mrgHaveLast) return s + ", \"last_frame\": null, \"last_group_num\": null, \"last_info\": null}";
    s += ", \"last_frame\": " + std::to_string(mrgLast.frame) + ", \"last_group_num\": " + std::to_string(mrgLast.groupNum) + ", \"last_info\": [";
    for (int k = 0; k < mrgLast.nMergeInfo && k < 256; ++k) {
        const cs_merge_info& m = mrgLast.info[k];
        s += std::string(k ? ", [" : "[") + std::to_string(m.frame1) + ", " + std::to_string(m.cam1) + ", " + std::to_string(m.gid1) + ", " +
             std::to_string(m.frame2) + ", " + std::to_string(m.cam2) + ", " + std::to_string(m.gid2) + "]";
    }
    s += "], \"last_nFeat\": [";
    for (int c = 0; c < nCams; ++c) s += (c ? ", " : "") + std::to_string(mrgLast.nFeat[c]);
    s += "]";
    auto table = [&](const char* name, auto at) {
        s += std::string(", \"") + name + "\": [";
        for (int a = 0; a < nCams; ++a) {
            s += a ? ", [" : "[";
            for (int b = 0; b < nCams; ++b) s += (b ? ", " : "") + std::to_string(at(a, b));
            s += "]";
        }
        s += "]";
    };
    table("last_nInCam", [&](int a, int b) { return mrgLast.nInCam[a][b]; });
    table("last_inNum", [&](int a, int b) { return mrgLast.inNum[a][b]; });
    table("last_fromTo", [&](int a, int b) { return (int)mrgLast.fromTo[a][b]; });
    return s + "}";
}

// CoSLAM::storeDynamicPoints + updateDisplayData of frame i where the reference has them (src/gui/CoSLAMThread.cpp:117-120): the tables as
// the registration left them, the poses just written, the frame's groups when the grouping runs
void FrameLoop::live_view(int i, int dsti) {
    const cs_camera_groups* g = o.grouping && grpCalls ? dGrpGroups + (int)((grpCalls - 1) % GROUP_RING) : nullptr;
    CSCHK(cs_liveview_frame_dev(live, (void*)poseS, i, nMap, dMapCount, dPf, dMapFlags, dMap, dR[dsti], dT[dsti], g));
    ++liveFrames;
    livePublished += i % o.liveEvery == 0;
}

// (behind the barrier) the newest snapshot's header and getDynTracks over the ring, as FrameLoop.live_stats of the Python loop
std::string FrameLoop::live_json() {
    if (!o.liveView) return "";
    const int dynCap = o.liveDynCap ? o.liveDynCap : std::max(1, nMap / 4);
    int nTr = 0, longest = 0;
    std::vector<int> ids(dynCap), lens(dynCap);
    std::vector<double> pts((size_t)dynCap * o.liveTrailDepth * 3);
    CSCHK(cs_liveview_trails(live, (void*)poseS, o.liveTrailDepth, dynCap, &nTr, ids.data(), lens.data(), pts.data()));
    for (int q = 0; q < nTr && q < dynCap; ++q) longest = std::max(longest, lens[q]);
    std::string s = "\"live_view\": {\"frames\": " + std::to_string(liveFrames) + ", \"frames_published\": " + std::to_string(livePublished) +
                    ", \"trails\": " + std::to_string(nTr) + ", \"longest_trail\": " + std::to_string(longest);
    const int newest = cs_liveview_newest(live);
    if (newest >= 0) {
        const cs_live_header* h = nullptr;
        const cs_live_point* p = nullptr;
        CSCHK(cs_liveview_fetch(live, newest, &h, &p));
        auto arr = [&](const int* a) {
            std::string r = "[";
            for (int c = 0; c < nCams; ++c) r += (c ? ", " : "") + std::to_string(a[c]);
            return r + "]";
        };
        s += ", \"frame\": " + std::to_string(h->frame) + ", \"nCur\": " + std::to_string(h->nCur) + ", \"nDyn\": " + std::to_string(h->nDyn) +
             ", \"curOverflow\": " + std::to_string(h->curOverflow) + ", \"dynOverflow\": " + std::to_string(h->dynOverflow) +
             ", \"curOverflowTotal\": " + std::to_string(h->curOverflowTotal) + ", \"dynOverflowTotal\": " + std::to_string(h->dynOverflowTotal) +
             ", \"nStatic\": " + std::to_string(h->counts.nStatic) + ", \"nDynamic\": " + std::to_string(h->counts.nDynamic) +
             ", \"nStaticFeat\": " + arr(h->counts.nStaticFeat) + ", \"nDynamicFeat\": " + arr(h->counts.nDynamicFeat) +
             ", \"bytes_per_published_frame\": " + std::to_string(sizeof(cs_live_header) + sizeof(cs_live_point) * (size_t)h->nCur);
    }
    return s + "}, ";
}

// first frame: detect, map association, first hand-back (GPUKLT::first + map initialisation stand-in)
void FrameLoop::first_frame() {
    for (int b = 0; b < 2; ++b) {
        HIPCHK(hipEventCreateWithFlags(&kltDone[b], hipEventDisableTiming));
        HIPCHK(hipEventCreateWithFlags(&destFree[b], hipEventDisableTiming));
    }
    dBar = dev_zeros<int>(64);
    const void* cur[16];
    void *dst[16], *cnt[16];
    for (int k = 0; k < nc; ++k) cur[k] = dFrames[c0 + k] + imgBytes * w.order[0], dst[k] = dDest[0][c0 + k], cnt[k] = dCnt[c0 + k];
    CSCHK(cs_klt_group_detect_dev(grp, cur, dst, cnt));
    CSCHK(cs_klt_group_advance(grp));
    CSCHK(cs_klt_group_synchronize(grp));
    if (o.world > 1) {   // every camera's first dest[] to every rank
        CSCHK(cs_exchange_allgather_dev(xchg, (void*)poseS, (const void* const*)dst, dR[0] + 9 * c0, dT[0] + 3 * c0));
        HIPCHK(hipDeviceSynchronize());
    }
    associate();
    CSCHK(cs_klt_handback_dev(o.dev, (void*)poseS, nc, hbOwn[0].data(), N, W, H, w.nColBlk, w.nRowBlk, PTS, 0));
    if (o.world > 1) CSCHK(cs_klt_handback_dev(o.dev, (void*)poseS, nCams - nc, hbOther.data(), N, W, H, w.nColBlk, w.nRowBlk, PTS, 0));
    HIPCHK(hipDeviceSynchronize());
    associate();  // (the first hand-back starts every track as new, i.e. unmapped: put the map back)
    HIPCHK(hipDeviceSynchronize());
    // frame 0 into the history as well (its pixels and poses: the first term of every track born in it, which a whole-track mergability
    // walk ends with); the dynamic test has nothing to say about one-frame tracks
    CSCHK(cs_detect_dynamic_dev(hist, (void*)poseS, 0, nCams, pu.data(), dR[0], dT[0], nMap, dMapFlags, 0, 20, 5, 3, 6.0, nullptr));
    HIPCHK(hipDeviceSynchronize());
    if (o.kfDrives) {   // nMappedPts of frame 0's key pose: the certainly static mapped features of the frame (enable_keyframe_decision, coslam_amd/frameloop.py)
        std::vector<int> st((size_t)nCams * N), sm((size_t)nCams * N), km(nCams, 0);
        std::vector<unsigned char> fl(nMap);
        HIPCHK(hipMemcpy(st.data(), dState, sizeof(int) * st.size(), hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(sm.data(), dS2M, sizeof(int) * sm.size(), hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(fl.data(), dMapFlags, fl.size(), hipMemcpyDeviceToHost));
        for (int c = 0; c < nCams; ++c)
            for (int q = 0; q < N; ++q) {
                const int sv = st[(size_t)c * N + q], m = sm[(size_t)c * N + q];
                if ((sv == 0 || sv == 1) && m >= 0 && m < nMap && (fl[m] & 7) == 0) ++km[c];
            }
        HIPCHK(hipMemcpy(dKfMapped, km.data(), sizeof(int) * nCams, hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(dKfSelfR, dR[0], sizeof(double) * 9 * nCams, hipMemcpyDeviceToDevice));
        HIPCHK(hipMemcpy(dKfSelfT, dT[0], sizeof(double) * 3 * nCams, hipMemcpyDeviceToDevice));
    }
    if (o.grouping) setup_camera_grouping();
    if (o.mergeCheck) setup_merge_check();
    if (o.liveView) {
        live = cs_liveview_create(o.dev, nCams, o.liveCurCap ? o.liveCurCap : nMap, o.liveDynCap ? o.liveDynCap : std::max(1, nMap / 4), o.liveDepth,
                                  o.liveTrailDepth, o.liveEvery);
        if (!live) {
            fprintf(stderr, "cs_liveview_create: %s\n", cs_last_error());
            exit(2);
        }
    }
}

// every tracked slot of the first frame onto the nearest projected map point within 1 px
void FrameLoop::associate() {
    std::vector<cs_klt_feature> d(N);
    std::vector<int> s2m(N);
    for (int c = 0; c < nCams; ++c) {
        const void* from = (c >= c0 && c < c0 + nc) ? (const void*)dDest[0][c] : (const void*)(xRecv + (size_t)c * xRecBytes);
        HIPCHK(hipMemcpy(d.data(), from, sizeof(cs_klt_feature) * N, hipMemcpyDeviceToHost));
        const std::vector<double>& uv = w.visUV[c];
        const int nv = (int)w.visIdx[c].size();
        for (int s = 0; s < N; ++s) {
            s2m[s] = -1;
            if (d[s].status < 0) continue;
            const double px = (double)d[s].pos[0] * W, py = (double)d[s].pos[1] * H;
            double best = 1.0;
            for (int q = 0; q < nv; ++q) {
                const double dx = uv[2 * q] - px, dy = uv[2 * q + 1] - py, dd = std::sqrt(dx * dx + dy * dy);
                if (dd < best) best = dd, s2m[s] = w.visIdx[c][q];
            }
        }
        HIPCHK(hipMemcpy(dS2M + (size_t)c * N, s2m.data(), sizeof(int) * N, hipMemcpyHostToDevice));
    }
}

// one frame: tracking, the apply of a due window, pose, NCC leg, registration, key-frame actions
void FrameLoop::step(int i, bool key) {
    const int orderLen = (int)w.order.size(), f = w.order[i % orderLen], fn = w.order[(i + 1) % orderLen], b = i & 1;
    const void *cur[16], *nxt[16];
    void *dst[16], *cnt[16];
    for (int k = 0; k < nc; ++k) {
        cur[k] = dFrames[c0 + k] + imgBytes * f, nxt[k] = dFrames[c0 + k] + imgBytes * fn;
        dst[k] = dDest[b][c0 + k], cnt[k] = dCnt[c0 + k];
    }
    if (i >= 2) HIPCHK(hipStreamWaitEvent(kltS, destFree[b], 0));
    CSCHK(cs_klt_group_prefetch_dev(grp, nxt));
    CSCHK(cs_klt_group_redetect_dev(grp, cur, dst, cnt));
    CSCHK(cs_klt_group_advance(grp));
    HIPCHK(hipEventRecord(kltDone[b], kltS));
    HIPCHK(hipStreamWaitEvent(poseS, kltDone[b], 0));
    const int src = (i + 1) & 1, dsti = i & 1;
    sched.apply_due(i, hist, pu.data(), dPf, nMap, dMap, dCov, dMapFlags, PIX, dR[src], dT[src]);
    CSCHK(cs_klt_handback_dev(o.dev, (void*)poseS, nc, hbOwn[b].data(), N, W, H, w.nColBlk, w.nRowBlk, PTS, i));
    CSCHK(cs_pose_intracam_batch_dev(o.dev, (void*)poseS, nc, PTS, dKall, dR[src] + 9 * c0, dT[src] + 3 * c0, dNpts + c0, nullptr,
                                     dMs + (size_t)c0 * PTS * 3, dms + (size_t)c0 * PTS * 2, 10.0, dR[dsti] + 9 * c0, dT[dsti] + 3 * c0,
                                     dOpt + c0, dOk + c0));
    if (o.world > 1) {
        // the merge step: every camera's {dest[], R, t} to every rank (ONE all-gather), the other ranks' poses into the pose arrays, their
        // cameras through the same hand-back
        CSCHK(cs_exchange_allgather_dev(xchg, (void*)poseS, (const void* const*)dst, dR[dsti] + 9 * c0, dT[dsti] + 3 * c0));
        CSCHK(cs_exchange_unpack_poses_dev(xchg, (void*)poseS, dR[dsti], dT[dsti], 1));
        CSCHK(cs_klt_handback_dev(o.dev, (void*)poseS, nCams - nc, hbOther.data(), N, W, H, w.nColBlk, w.nRowBlk, PTS, i));
    }
    // parallelPoseUpdate(false): the gate + seqTriangulate loop of poseUpdate3D, detectDynamicFeaturePoints(20, 5, 3, MAX_EPI_ERR)
    // and mapPointsClassify(12.0) (SL_CoSLAM.cpp:385): the uncertain / dynamic points of this frame decided again -- CoSLAM::poseUpdate as two
    // launches (the gate's lane of a point also lists it for the classification)
    CSCHK(cs_pose_update_classify_frame_dev(hist, (void*)poseS, pu.data(), dPf, nMap, dR[dsti], dT[dsti], dMap, dCov, dMapFlags, 0, PIX, i, 20, 5,
                                            3, 6.0, nullptr, nullptr, nullptr, nullptr, nullptr, dNewPt, dSfn, dFirstFrm, PIX_CLASSIFY, nullptr));
    if (o.grouping) camera_grouping(i, dsti);   // cameraGrouping: behind poseUpdate, before activeMapPointsRegister
    if (o.kfDrives)   // genNewMapPoints' first half (:1294-1346): is a camera ready for a key frame; addKeyFrame's bookkeeping when `decrease` holds
        CSCHK(cs_keyframe_ready_dev(o.dev, (void*)poseS, nCams, N, kfCams[dsti].data(), nMap, dMap, dMapFlags, dFirstFrm, i, o.kfRatio, 5.0,
                                    kfMinTranslation, 1, dKfReady, dKfCnt, dKfCen, dKfStats));
    // genNewMapPoints every 4th frame -- BEFORE currentMapPointsRegister, as in the reference's frame (src/gui/CoSLAMThread.cpp:104-118):
    // the new map points take their features before the current points' registration looks at them
    if (nCams >= 2 && i % NCC_EVERY == 0) ncc_leg(i, f, dsti);
    register_frame(i, dsti);
    // the tracker of frame i + 2 is released at the END of the frame's pose work (released right behind the hand-back it runs two frames
    // ahead and under more of the pose stream's kernels: -10 %, profiles/r04_ab_runs.txt)
    HIPCHK(hipEventRecord(destFree[b], poseS));
    if (o.liveView) live_view(i, dsti);   // storeDynamicPoints + updateDisplayData: the end of the frame, behind the tracker's release
    if (o.kfDrives)
        keyframe_decision_step(i, dsti);
    else if (key)
        key_frame_actions(i, hb[b].data(), dR[dsti], dT[dsti], false, dsti);
}

// NewMapPtsNCC::addSlam's features: this frame's, on tracks of more than three frames, unmapped or on a false point; the whole run in a
// handful of launches: resize + cutter of all cameras, the passing pairs of all camera pairs, then seeds + disparity guide + greedy matches,
// featTracksFromMatches, reconstructTracks, output: new points behind *dMapCount
void FrameLoop::ncc_leg(int i, int f, int dsti) {
    CSCHK(cs_ncc_candidate_mask_dev(o.dev, (void*)poseS, nCams, N, dState, dS2M, dSpan, dMapFlags, nMap, 3, dValid, 0));
    for (int c = 0; c < nCams; ++c) ncams[c].img = dFrames[c] + imgBytes * f;
    // the blocks of the rank's own cameras (it holds their images); N > 1: blocks and line coefficients of every camera to every
    // rank (two all-gathers in place, 256 + 64 KB per camera, every 4th frame); the candidate masks come from replicated state
    CSCHK(cs_ncc_get_blocks_group_dev(o.dev, (void*)poseS, nc, ncams.data() + c0, W, H, N, 0.3));
    if (o.world > 1) {
        CSCHK(cs_comm_allgather_dev(comm, (void*)poseS, dBlk + (size_t)c0 * N * 128, dBlk, (size_t)nc * N * 128));
        CSCHK(cs_comm_allgather_dev(comm, (void*)poseS, dAbc + (size_t)c0 * N * 4, dAbc, sizeof(double) * (size_t)nc * N * 4));
    }
    CSCHK(cs_ncc_fmats_dev(o.dev, (void*)poseS, nCams, nCams - 1, pairA.data(), pairB.data(), pairIK.data(), dR[dsti], dT[dsti], dFm));
    CSCHK(cs_ncc_epi_pairs_group_dev(o.dev, (void*)poseS, nCams, ncams.data(), N, nCams - 1, jobs.data(), 50.0, 0.80, NCC_PAIR_CAP));
    CSCHK(cs_newpts_from_pairs_dev(o.dev, (void*)poseS, nCams, N, pu.data(), pairPtr.data(), cntPtr.data(), NCC_PAIR_CAP, dR[dsti], dT[dsti],
                                   dMap, dCov, dMapFlags, dNewPt, dFirstFrm, dPf, nMap, dMapCount, i, 80.0, 3.0, PIX, 2, W, H, dNpScratch,
                                   dNpCounts));
    ++nccRuns;
}

// currentMapPointsRegister: the search over a list of map points, the whole-track mergability, the decisions, refineMapPoint, and the
// reference's SECOND VISITS (SL_CoSLAM.cpp:864-869, :889-893): the points that registered are refined and visited again in their next
// camera's loop -- rounds of list + search + whole-track mergability + walks + refine over just those points, every rank for ALL cameras
// on its replica (cs_register_revisit_*; tools/r06_exact_vs_single.py: with two rounds the map is the reference order's, frame after frame)
void FrameLoop::register_frame(int i, int dsti) {
    // one search pass over `list` (P entries) for cameras cam0 .. cam0 + nRun - 1; the tables are indexed by the map index
    auto search = [&](int P, const int* list, int cam0, int nRun) {
        cs_register_pass ps;
        memset(&ps, 0, sizeof(ps));
        ps.P = P, ps.sigmaSearch = PIX, ps.maxDist = 3 * PIXVAR, ps.sigmaMerge = PIX;   // (maxDist: a common scale of a search's distances)
        ps.M = dMap, ps.cov = dCov, ps.pointFeat = dPf, ps.list = list;
        ps.mapFlags = dMapFlags, ps.maxDistDynamic = 4 * PIXVAR;   // (the certainly dynamic points' scale: SL_CoSLAM.cpp:973)
        ps.slot = reg.slot, ps.m = reg.m, ps.var = reg.var, ps.dist = reg.dist, ps.flags = reg.flags;
        CSCHK(cs_register_search_passes_range_dev(o.dev, (void*)poseS, nCams, cam0, nRun, rc[dsti].data(), N, W, H, 1, &ps));
    };
    // refineMapPoint of the points that gained a feature: with the references brought up to this frame first (tracked on / first feature /
    // re-linked behind an older one / stale / detached: cs_feat_ref_advance_dev, idempotent within a frame)
    auto refine = [&]() {
        CSCHK(cs_feat_ref_advance_dev(hist, (void*)poseS, pu.data(), nMap, dPf, i, dFref, dRstat, dFrefCnt));
        CSCHK(cs_refine_map_points_ref_dev(hist, (void*)poseS, pu.data(), dFref, nMap, dRegged, dMap, dCov, PIX, nullptr));
    };
    // search step: curMapPts of this frame as a list (the points with a feature of this frame, wherever they sit in the map -- the ones
    // genNewMapPoints just appended included), ONE pass over it for the own cameras' columns.  (activeMapPointsRegister's search is not run:
    // the reference's attach loop behind it cannot be reached, tests/cxx/ref_active_test.cpp)
    CSCHK(cs_register_list_current_cap_dev(o.dev, (void*)poseS, nCams, nMap, dMapCount, dPf, dMapFlags, dCurList, dCurCount, reg.slot, P_REG, dCurOverflow));
    search(P_REG, dCurList, c0, nc);
    // staticCheckMergability of the candidates over their WHOLE tracks (SL_CoSLAM.cpp:714-729, :768) as a running verdict
    CSCHK(cs_register_mergability_running_list_dev(hist, (void*)poseS, c0, nc, pu.data(), nMap, dCurList, P_REG, dMap, dCov, reg.slot, reg.flags, PIX,
                                                   0.5, dMergeCache, dMergeable, dMergeRun));
    if (o.world > 1) {
        // the own cameras' columns of the candidate tables (the listed rows only) to every rank: ONE all-gather, then every rank takes the
        // same decisions on its replica
        CSCHK(cs_register_candidates_pack_list_dev(o.dev, (void*)poseS, P_REG, nCams, c0, nc, dCurList, reg.slot, reg.flags, dMergeable, dCandSend));
        CSCHK(cs_comm_allgather_dev(comm, (void*)poseS, dCandSend, dCandRecv, sizeof(int) * (size_t)3 * nc * P_REG));
        CSCHK(cs_register_candidates_unpack_list_dev(o.dev, (void*)poseS, P_REG, nCams, nc, o.rank, dCurList, dCandRecv, reg.slot, reg.flags, dMergeable));
    }
    // every 50th frame with bMerge (CoSLAMThread.cpp:117-118): the static points' walks one after the other, checkUnify at a conflict; then
    // the certainly dynamic points (kind 2) -- and no second visits
    if (i % 50 == 0) {
        CSCHK(cs_register_decide_merge_list_dev(hist, (void*)poseS, pu.data(), nMap, 0, dCurList, P_REG, reg.slot, reg.flags, dMergeable, dMapFlags, dPf, dMap,
                                                dCov, PIX, dAttached, dRegged, dMergeScratch, dMergeCnt, /*onlyCam*/ -1));
        refine();
        ++nMergeFrames;
        CSCHK(cs_register_decide_kinds_dev(o.dev, (void*)poseS, nCams, N, nMap, 0, reg.slot, reg.flags, dMergeable, dMapFlags, dPf, s2mPtrs.data(),
                                           dAttached, dRegged, dDecScratch, /*nSweeps: until settled*/ 0, dDecCnt, /*onlyCam*/ -1, 2));
        refine();
        return;
    }
    if (o.fusedRounds) {
        // the decision (curStaticPointsRegInGroup, bMerge false: who attaches which feature) with the second visits' lists built by the walks
        // themselves and advance + refine as one launch: 2 launches instead of 3 behind the single pass; then every round of the second visits
        // as ONE launch of one workgroup, which leaves at once when list 0 is empty -- the usual frame (cs_register_decide_kinds_rounds_dev,
        // cs_feat_ref_advance_refine_dev, cs_register_revisit_rounds_dev: the bytes of a search, a mergability, a walk and an advance + refine
        // launch per round)
        CSCHK(cs_register_decide_kinds_rounds_dev(o.dev, (void*)poseS, nCams, N, nMap, 0, reg.slot, reg.flags, dMergeable, dMapFlags, dPf, s2mPtrs.data(),
                                                  dAttached, dRegged, dDecScratch, 0, dDecCnt, -1, 3, dRvLists, RV_CAP, RV_ROUNDS, dRvCounts, dRvVisit,
                                                  dRvNext));
        CSCHK(cs_feat_ref_advance_refine_dev(hist, (void*)poseS, pu.data(), nMap, dPf, i, dFref, dRstat, dFrefCnt, dCurList, P_REG, 1, dRegged, 0, dMap, dCov, PIX));
        cs_register_pass ps;
        memset(&ps, 0, sizeof(ps));
        ps.P = RV_CAP, ps.sigmaSearch = PIX, ps.maxDist = 3 * PIXVAR, ps.sigmaMerge = PIX;
        ps.M = dMap, ps.cov = dCov, ps.pointFeat = dPf, ps.mapFlags = dMapFlags, ps.maxDistDynamic = 4 * PIXVAR;
        ps.slot = reg.slot, ps.m = reg.m, ps.var = reg.var, ps.dist = reg.dist, ps.flags = reg.flags;
        CSCHK(cs_register_revisit_rounds_dev(hist, (void*)poseS, rc[dsti].data(), pu.data(), W, H, &ps, nMap, i, 0, 3, dMap, dCov, PIX, 0.0, dMergeCache,
                                             dMergeable, dRvLists, dRvCounts, RV_CAP, RV_ROUNDS, dRvVisit, dRvNext, dMapFlags, dPf, s2mPtrs.data(),
                                             dAttached, dRvReg[0], dDecScratch, dCurList, dCurCount, P_REG, dRvCnt, dFref, dRstat, dFrefCnt));
        return;
    }
    // the same launch per step: the decision of the certainly static points, behind them the certainly dynamic ones (kinds 3), one call;
    // then the rounds of second visits, each listing the points the last one registered
    CSCHK(cs_register_decide_kinds_dev(o.dev, (void*)poseS, nCams, N, nMap, 0, reg.slot, reg.flags, dMergeable, dMapFlags, dPf, s2mPtrs.data(),
                                       dAttached, dRegged, dDecScratch, /*nSweeps: until settled*/ 0, dDecCnt, /*onlyCam*/ -1, 3));
    refine();
    unsigned char* regIn = dRegged;
    for (int r = 0; r < RV_ROUNDS; ++r) {
        unsigned char* regOut = dRvReg[r & 1];
        CSCHK(cs_register_revisit_list_dev(o.dev, (void*)poseS, nCams, nMap, RV_CAP, r == 0, dPf, dAttached, regIn, r == 0, regOut, dRvVisit, dRvNext, dRvList,
                                           dRvListCnt));
        search(RV_CAP, dRvList, 0, nCams);
        CSCHK(cs_register_mergability_running_list_dev(hist, (void*)poseS, 0, nCams, pu.data(), nMap, dRvList, RV_CAP, dMap, dCov, reg.slot, reg.flags,
                                                       PIX, 0.0, dMergeCache, dMergeable, nullptr));
        CSCHK(cs_register_revisit_decide_dev(o.dev, (void*)poseS, nCams, N, nMap, RV_CAP, 0, 3, dRvList, dRvNext, dRvVisit, reg.slot, reg.flags, dMergeable,
                                             dMapFlags, dPf, s2mPtrs.data(), dAttached, regOut, dDecScratch, dCurList, dCurCount, P_REG, dRvCnt, dRvListCnt));
        CSCHK(cs_feat_ref_advance_list_dev(hist, (void*)poseS, pu.data(), nMap, dPf, i, dFref, dRstat, dFrefCnt, dRvList, RV_CAP));
        CSCHK(cs_refine_map_points_ref_dev(hist, (void*)poseS, pu.data(), dFref, nMap, regOut, dMap, dCov, PIX, nullptr));
        regIn = regOut;
    }
}

// a key frame's actions: the inter-camera solve, the frame's records and poses into the window's ring, the window's request
void FrameLoop::key_frame_actions(int f, const cs_handback_cam* cams, const double* Rk, const double* tk, bool placed, int dsti) {
    // InterCamPoseEstimator::addMapPoints + apply: every camera's current pose, the block-voted static features' map points fixed, the dynamic
    // points free; sigma 6, 3 x 40 (key frame k's inter-camera solve on rank (k + world / 2) % world, its window on rank k % world: the two
    // chains on different GPUs)
    if ((nKey + o.world / 2) % o.world == o.rank)
        CSCHK(cs_ba_solve_intercam_async(icWs, icam, (void*)poseS, icCams.data(), W, H, w.nColBlk, w.nRowBlk, dR[dsti], dT[dsti], dMap, dMapFlags,
                                         dNewPt, dPf, 6.0, 3, 40));
    ++nKey;
    if (o.mergeCheck) merge_check(f, cams, Rk, tk);   // CoSLAM::mergeCamGroups' gate at the key frame (genNewMapPoints, :1339-1342)
    CSCHK(cs_ba_window_push_dev(win, (void*)poseS, cams, dK, 1, Rk, tk, f));
    sched.request(f, placed, dMap, dMapFlags);
}

// this frame's decision word, records and poses into slot i % (LAG + 1) of the ring (no host wait), then the decision of frame i - LAG
void FrameLoop::keyframe_decision_step(int i, int dsti) {
    const int ring = o.kfLag + 1;
    KfSnap& sn = kfRing[i % ring];
    CSCHK(cs_keyframe_snapshot_dev(o.dev, (void*)poseS, nCams, N, dXY, dState, dS2M, dR[dsti], dT[dsti], dKfReady + nCams + 1, sn.xy, sn.st, sn.s2m, sn.R,
                                   sn.t, sn.word));
    HIPCHK(hipEventRecord(sn.ev, poseS));
    sn.frame = i;
    const int f = i - o.kfLag;
    KfSnap& old = kfRing[((f % ring) + ring) % ring];
    if (f >= 1 && old.frame == f) {
        HIPCHK(hipEventSynchronize(old.ev));   // (a frame LAG behind: fired long ago unless the host has caught up with the device)
        if (*old.word) {
            kfPlaced.push_back(f);
            key_frame_actions(f, old.hb.data(), old.R, old.t, true, dsti);
        }
    }
}

// a window / a rig that holds no usable point (every map point of its key frames false, say: the closed orbit starves after some thousands
// of frames) is a solve with nothing to do -- it packed an empty record (ok = 0, applies nothing) -- not a failure of the
// loop: counted (coslam_amd/frameloop.py: drain())
void FrameLoop::wait_ws(cs_ba* ws) {
    for (;;) {
        const int rc = cs_ba_wait(ws);
        if (rc == CS_OK) return;
        const char* e = cs_last_error();
        if (e && (strstr(e, "no map point has two feature points") || strstr(e, "no static feature point carries a map point"))) {
            ++nEmptySolves;
            continue;   // (the worker goes on with the next request: wait again)
        }
        fprintf(stderr, "cs_ba_wait failed (%d): %s\n", rc, e ? e : "?");
        exit(3);
    }
}

void FrameLoop::barrier() {
    wait_ws(icWs);
    wait_ws(jointWs);
    HIPCHK(hipDeviceSynchronize());
    if (o.world > 1) {   // every rank has drained: a small all-gather as the barrier between the ranks
        CSCHK(cs_comm_allgather_dev(comm, (void*)poseS, dBar + o.rank, dBar, sizeof(int)));
        HIPCHK(hipDeviceSynchronize());
    }
}

// the JSON line: the rate, what was computed (live features, pose flags, the solves' statistics) and the digest
void FrameLoop::report(double dt, double dtHost, int applied0, const int rvCnt0[4]) {
    const int steps = o.steps;
    int okAll = 1, minLive = N;
    {
        std::vector<int> ok(nCams);
        HIPCHK(hipMemcpy(ok.data(), dOk, sizeof(int) * nCams, hipMemcpyDeviceToHost));
        for (int c = c0; c < c0 + nc; ++c) okAll &= (ok[c] != 0);   // (the rank's own cameras: it solves their poses)
        std::vector<cs_klt_feature> d(N);
        const int last = nDone & 1;
        for (int c = c0; c < c0 + nc; ++c) {
            HIPCHK(hipMemcpy(d.data(), dDest[last][c], sizeof(cs_klt_feature) * N, hipMemcpyDeviceToHost));
            int live = 0;
            for (const cs_klt_feature& q : d) live += q.status >= 0;
            minLive = std::min(minLive, live);
        }
    }
    cs_ba_stats sj, si;
    memset(&sj, 0, sizeof(sj)), memset(&si, 0, sizeof(si));
    int jC = 0, jP = 0, jO = 0;
    CSCHK(cs_ba_window_last_problem(win, &jC, &jP, &jO, nullptr, nullptr));
    if (sched.nMySolves > 0) CSCHK(cs_ba_download(jointWs, jC, jP, jO, nullptr, nullptr, nullptr, nullptr, &sj));   // (a rank solves every world-th window)
    int iC = 0, iP = 0, iO = 0, iS = 0;
    CSCHK(cs_ba_intercam_last_problem(icam, &iC, &iP, &iO, &iS, nullptr));
    if (iC > 0) CSCHK(cs_ba_download(icWs, iC, iP, iO, nullptr, nullptr, nullptr, nullptr, &si));
    // the state every rank must agree on after the last frame (and a one-rank run must reproduce): FNV-1a over the map points in use, their
    // flags, every camera's slot -> point table and track spans, the current poses
    unsigned long long digest = 1469598103934665603ull;
    int mapCountNow = 0;
    HIPCHK(hipMemcpy(&mapCountNow, dMapCount, sizeof(int), hipMemcpyDeviceToHost));
    auto eat = [&](const void* dptr, size_t bytes) {
        std::vector<unsigned char> h(bytes);
        HIPCHK(hipMemcpy(h.data(), dptr, bytes, hipMemcpyDeviceToHost));
        for (unsigned char v : h) digest = (digest ^ v) * 1099511628211ull;
    };
    eat(dMap, sizeof(double) * 3 * (size_t)mapCountNow), eat(dCov, sizeof(double) * 9 * (size_t)mapCountNow), eat(dMapFlags, (size_t)mapCountNow);
    eat(dS2M, sizeof(int) * (size_t)nCams * N), eat(dSpan, sizeof(int) * (size_t)nCams * 2 * N);
    eat(dR[nDone & 1], sizeof(double) * 9 * nCams), eat(dT[nDone & 1], sizeof(double) * 3 * nCams);
    int npCounts[4] = {0, 0, 0, 0};
    HIPCHK(hipMemcpy(npCounts, dNpCounts, sizeof(npCounts), hipMemcpyDeviceToHost));
    int curOverflow = 0;
    HIPCHK(hipMemcpy(&curOverflow, dCurOverflow, sizeof(int), hipMemcpyDeviceToHost));
    int rvCnt[4] = {0, 0, 0, 0}, rvListCnt[4] = {0, 0, 0, 0};
    HIPCHK(hipMemcpy(rvCnt, dRvCnt, sizeof(rvCnt), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(rvListCnt, dRvListCnt, sizeof(rvListCnt), hipMemcpyDeviceToHost));
    if (o.fusedRounds) HIPCHK(hipMemcpy(&rvListCnt[1], dRvCounts + RV_ROUNDS, sizeof(int), hipMemcpyDeviceToHost));
    std::string placedJson = "[";
    for (size_t q = 0; q < kfPlaced.size(); ++q) placedJson += (q ? ", " : "") + std::to_string(kfPlaced[q]);
    placedJson += "]";
    int decUnsettled = 0;   // (the decision scratch's last int: sticky "some call's sweeps did not settle")
    HIPCHK(hipMemcpy(&decUnsettled, (char*)dDecScratch + cs_register_decide_scratch_bytes(nCams, N, nMap) - sizeof(int), sizeof(int),
                     hipMemcpyDeviceToHost));
    const std::string groupingJson = grouping_json(), mergeJson = merge_json(), liveJson = live_json();
    const char* transport = o.world == 1 ? "none" : o.hostSegment ? "host segment (test)" : "rccl";
    printf("{\"frames_per_s\": %.3f, \"ms_per_step\": %.5f, \"steps\": %d, \"warmup\": %d, \"host_enqueue_ms_per_step\": %.5f, "
           "\"cams_per_tracker_launch\": %d, \"pose_ok\": %s, \"min_live_features\": %d, \"joint_lm_steps\": %d, \"joint_cost\": %.6f, "
           "\"intercam_lm_steps\": %d, \"intercam_cost\": %.6f, \"ncc_runs\": %d, \"joint_ba_from_window\": true, \"joint_cameras\": %d, "
           "\"joint_points\": %d, \"joint_measurements\": %d, \"ba_lag\": %d, \"windows_applied_in_timed_region\": %d, \"apply_wait_errors\": %d, "
           "\"intercam_static_points\": %d, \"intercam_dynamic_points\": %d, \"map_points_at_start\": %d, \"map_points_in_use\": %d, "
           "\"map_capacity\": %d, \"new_map_points_last_run\": %d, \"register_decisions_unsettled\": %s, \"bmerge_frames\": %d, \"current_points_beyond_the_cap\": %d, \"second_visit_rounds\": %d, \"second_visit_features_attached\": %d, "
           "\"second_visit_conflicts\": %d, \"second_visit_conflicts_in_timed_region\": %d, \"second_visit_points_beyond_the_list\": %d, "
           "\"key_frames_placed_by_the_decision\": %s, \"keyframe_lag\": %d, \"frames_run\": %d, \"windows_requested\": %lld, \"windows_applied\": %d, \"windows_not_applied_history_too_short\": %d, "
           "\"camera_grouping\": %s, \"merge_check\": %s, %s\"rank\": %d, \"world\": %d, \"cameras_per_rank\": %d, \"transport\": \"%s\", \"digest\": \"%016llx\"}\n",
           steps / dt, dt / steps * 1e3, steps, o.warmup, dtHost / steps * 1e3, w.camsPerLaunch, okAll ? "true" : "false", minLive,
           sj.nIterTotal, sj.cost, si.nIterTotal, si.cost, nccRuns, jC, jP, jO, o.baLag, sched.nApplied - applied0,
           cs_ba_output_wait_errors(bout), iS, iP - iS, w.nPts, mapCountNow, nMap, npCounts[0], decUnsettled ? "true" : "false", nMergeFrames, curOverflow,
           RV_ROUNDS, rvCnt[0], rvCnt[2], rvCnt[2] - rvCnt0[2], rvListCnt[1], o.kfDrives ? placedJson.c_str() : "null", o.kfDrives ? o.kfLag : 0, nDone,
           sched.nRequested, sched.nApplied, sched.nNotApplied, groupingJson.c_str(), mergeJson.c_str(), liveJson.c_str(), o.rank, o.world, nc, transport, digest);
    fflush(stdout);
}

// CoSLAM::exportResults behind the loop (reference src/gui/CoSLAMThread.cpp): the six result files into COSLAM_EXPORT_DIR from the device
// state, after the drain; every rank holds the same map and history, rank 0 writes.  A failure ends the process with status 3.
void FrameLoop::export_results() {
    if (o.rank != 0) return;
    const double kc[5] = {0, 0, 0, 0, 0};
    std::vector<std::string> paths(nCams);
    std::vector<cs_loop_export_cam> cams(nCams);
    for (int c = 0; c < nCams; ++c) {
        paths[c] = "camera_" + std::to_string(c);
        cams[c] = cs_loop_export_cam{paths[c].c_str(), w.K.data(), kc, W, H, 0};
    }
    long long stats[3] = {0, 0, 0};
    const auto t0 = std::chrono::steady_clock::now();
    CSCHK(cs_loop_export_results(o.exportDir, hist, (void*)poseS, dFref, nMap, dMap, dCov, dMapFlags, cams.data(), 1, stats));
    const double dt = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    fprintf(stderr, "[frame_loop] exported frames %d..%d (%d archived), %lld static points, %lld features (%lld from the archive) to %s in %.3f s\n",
            cs_track_history_first_frame(hist), cs_track_history_newest_frame(hist), cs_track_history_archive_frames(hist), stats[0], stats[1],
            stats[2], o.exportDir, dt);
}

int main(int argc, char** argv) {
    const Options opt = read_options(argc, argv);
    Reader rd{nullptr};
    Workload wl = read_header(opt, rd);
    check_config(opt, wl);
    // the device comes up BEFORE the frames are read: how long the runtime has been up when the streams are created decides which of
    // them share a hardware queue.  With the joint BA's stream on the tracker stream's queue, the tracker's event wait sits in front of
    // the solve that the pose stream's device wait for a BA record needs, and every such wait runs into its time limit
    HIPCHK(hipSetDevice(opt.dev));
    read_body(rd, wl);
    FrameLoop loop(opt, wl);
    loop.setup_trackers(wl.frames);
    loop.setup_state();
    if (opt.world > 1) loop.setup_comm();
    loop.setup_registration();
    loop.setup_cameras();
    loop.setup_keyframe_solves();
    loop.setup_keyframe_decision();
    loop.setup_window_records();
    loop.setup_ncc();
    loop.setup_decision_scratch();
    loop.first_frame();

    // set-up (one key-frame interval: graph capture in the BA workers, lazy code-object loading), warm-up, timed loop (with the window: 5
    // key-frame intervals, so that every timed solve has its 5 key frames = 5 x nCams cameras); the frame sequence runs on through set-up,
    // warm-up and the timed region
    const int ke = std::max(wl.keyEvery, 1);
    loop.run(WIN_KF * ke + 1);
    loop.barrier();
    loop.run((ke - loop.nDone % ke) % ke);
    loop.run(4 * ke);   // (one set-up round: bench.py --setup-rounds 1)
    loop.barrier();
    if (opt.timedFrom - opt.warmup - 1 > loop.nDone) {   // untimed, like bench.py's set-up loop: up to where its warm-up started
        loop.run(opt.timedFrom - opt.warmup - 1 - loop.nDone);
        loop.barrier();
    }
    loop.run(opt.warmup);
    loop.barrier();
    const int applied0 = loop.sched.nApplied;
    int rvCnt0[4] = {0, 0, 0, 0};   // (the second visits' counters at the start of the timed region)
    HIPCHK(hipMemcpy(rvCnt0, loop.dRvCnt, sizeof(rvCnt0), hipMemcpyDeviceToHost));
    const auto t0 = std::chrono::steady_clock::now();
    loop.run(opt.steps);
    const auto t1 = std::chrono::steady_clock::now();
    loop.barrier();
    const auto t2 = std::chrono::steady_clock::now();
    loop.report(std::chrono::duration<double>(t2 - t0).count(), std::chrono::duration<double>(t1 - t0).count(), applied0, rvCnt0);
    if (opt.exportDir) loop.export_results();

    if (loop.xchg) cs_exchange_destroy(loop.xchg);
    if (loop.comm) cs_comm_destroy(loop.comm);
    return 0;
}
