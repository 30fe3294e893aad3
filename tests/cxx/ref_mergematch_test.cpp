// ref_mergematch_test.cpp -- the reference's OWN MergeCameraGroup::storeFeaturePoints (src/app/SL_MergeCameraGroup.cpp:179-188),
// matchFeaturePointsNCC (:262-307, with getScaledNCCBlocks / getNCCBlock of src/slam/SL_NCCBlock.cpp, getEpiNccMat of
// src/slam/SL_FeatureMatching.cpp and matchNCCBlock) and the loop of matchMergableCameras (:320-421), on KeyFrame / KeyPose / FeaturePoint
// objects built from scene files: the fixture that pins cs_merge_match_run_dev and cs_merge_match_select.
//
// Stand-ins that replay a scene's recorded inputs and compute nothing: detectSURFPoints (the point list of the camera whose image it is
// given), matchSurf (the entry's SURF matches), estimateEMat (the entry's E), evaluateEMat (the entry's inlier flags).  genMergeInfoVer2 at
// :416 is redirected on the compile line to refRecordGenMergeInfo, a recorder of its five arguments.  Un-vendored on the path and OUR
// definitions (csrc/newpts.hip:15-21): getDisparityMat, greedyGuidedNCCMatch, getMatchedPts; vecFeatPt2Mat is the reference's own
// template.  The OpenCV cutter is oracle/ref_shim's restatement.  Besides the loop the driver calls matchFeaturePointsNCC itself for every
// entry the loop would match, so that the matches of EVERY job are recorded (the loop keeps them in a local array), and forms F with the
// functions matchFeaturePointsNCC forms it with (F is a local there).
//   ref_mergematch_test golden <in.bin> <out.bin>          CPU only
// Built by oracle/Makefile, target _ref/ref_mergematch_test (where the reference tree exists; SL_MergeCameraGroup.cpp goes through
// ref_mergeconstraints_test's three rewrites and a fourth that redirects :416).
// TEST INFRASTRUCTURE; the binary goes to oracle/_ref/ (untracked), nothing on the GPU side needs it.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <vector>

#include "app/SL_MergeCameraGroup.h"
#include "geometry/SL_Geometry.h"
#include "math/SL_LinAlg.h"
#include "slam/SL_KeyPoseList.h"

// ---- un-vendored helpers named by the file but off this path ----
void sortWithInd(int, int*, int*, bool) { abort(); }
void matEyes(int, Mat_d&) { abort(); }
void matZeros(int, int, Mat_d&) { abort(); }
void bundleAdjustRobust(int, std::vector<Mat_d>&, std::vector<Mat_d>&, std::vector<Mat_d>&, int, std::vector<Point3d>&,
                        std::vector<std::vector<Meas2D> >&, double, int, int) {
    abort();
}

// ---- un-vendored on the path: our definitions ----
void getMatchedPts(const Matching& matches, const Mat_d& pts1, const Mat_d& pts2, Mat_d& m1, Mat_d& m2) {
    m1.resize(matches.num, 2), m2.resize(matches.num, 2);
    for (int k = 0; k < matches.num; ++k) {
        m1.data[2 * k] = pts1.data[2 * matches[k].idx1], m1.data[2 * k + 1] = pts1.data[2 * matches[k].idx1 + 1];
        m2.data[2 * k] = pts2.data[2 * matches[k].idx2], m2.data[2 * k + 1] = pts2.data[2 * matches[k].idx2 + 1];
    }
}
void getDisparityMat(const Mat_d& c1, const Mat_d& c2, const Mat_d& s1, const Mat_d& s2, double maxDisp, Mat_d& disp) {
    const int M = c1.rows, N = c2.rows, S = s1.rows;
    disp.resize(M, N);
    for (int i = 0; i < M; ++i) {
        const double x1 = c1.data[2 * i], y1 = c1.data[2 * i + 1];
        double best = 1.0e300;
        int bk = 0;
        for (int k = 0; k < S; ++k) {
            const double dx = s1.data[2 * k] - x1, dy = s1.data[2 * k + 1] - y1, d2 = dx * dx + dy * dy;
            if (d2 < best) best = d2, bk = k;
        }
        for (int j = 0; j < N; ++j) {
            if (!S) {
                disp.data[(size_t)i * N + j] = 0;   // no seeds: no guide
                continue;
            }
            const double ex = (c2.data[2 * j] - x1) - (s2.data[2 * bk] - s1.data[2 * bk]);
            const double ey = (c2.data[2 * j + 1] - y1) - (s2.data[2 * bk + 1] - s1.data[2 * bk + 1]);
            const double d = sqrt(ex * ex + ey * ey);
            disp.data[(size_t)i * N + j] = (d <= maxDisp) ? d : -1.0;
        }
    }
}
struct Cand {
    double s;
    int i, j;
};
int greedyGuidedNCCMatch(const Mat_d& ncc, const Mat_d& disp, Matching& matches) {
    const int M = ncc.rows, N = ncc.cols;
    std::vector<Cand> c;
    for (int i = 0; i < M; ++i)
        for (int j = 0; j < N; ++j)
            if (ncc.data[(size_t)i * N + j] >= 0 && disp.data[(size_t)i * N + j] >= 0) {
                const Cand q = {ncc.data[(size_t)i * N + j], i, j};
                c.push_back(q);
            }
    std::sort(c.begin(), c.end(), [](const Cand& a, const Cand& b) { return a.s > b.s || (a.s == b.s && (a.i < b.i || (a.i == b.i && a.j < b.j))); });
    std::vector<char> ru(M, 0), cu(N, 0);
    matches.clear();
    for (size_t q = 0; q < c.size(); ++q) {
        if (ru[c[q].i] || cu[c[q].j]) continue;
        ru[c[q].i] = cu[c[q].j] = 1;
        matches.add(c[q].i, c[q].j, c[q].s);
    }
    return matches.num;
}
int greedyNCCMatch(const Mat_d&, Matching&) { abort(); }

// ---- OpenCV, as getNCCBlock names it (oracle/ref_shim/ref_not_on_path.h declares the types without state): the constructors note their
// arguments, cv::getRectSubPix is the oracle's restatement of the 8u -> 8u path (oracle/ncc_oracle.c, liboracle.so) ----
extern "C" void onc_get_rect_sub_pix_u8(const unsigned char* img, int W, int H, double cx, double cy, int win, unsigned char* patch);
namespace {
struct CvNote {
    int rows, cols;
};
std::map<const cv::Mat*, CvNote> g_cvMat;
int g_cvW = 0, g_cvH = 0;
double g_cvX = 0, g_cvY = 0;
unsigned char g_cvPatch[32 * 32];
}  // namespace
cv::Size::Size() {}
cv::Size::Size(int w, int h) { g_cvW = w, g_cvH = h; }
cv::Point2d::Point2d(double x, double y) { g_cvX = x, g_cvY = y; }
cv::Mat::Mat() : data(0) {}
cv::Mat::Mat(int rows, int cols, int, void* d) : data((unsigned char*)d) {
    const CvNote n = {rows, cols};
    g_cvMat[this] = n;
}
void cv::getRectSubPix(cv::Mat& img, cv::Size, cv::Point2d, cv::Mat& patch) {
    const CvNote n = g_cvMat[&img];
    if (g_cvW != g_cvH || g_cvW > 32 || !n.rows) abort();
    onc_get_rect_sub_pix_u8(img.data, n.cols, n.rows, g_cvX, g_cvY, g_cvW, g_cvPatch);
    patch.data = g_cvPatch;
}

// ---- the scene, and the stand-ins that replay it ----
struct Entry {
    int iCam, gId1, jCam, gId2, nMatch;
    std::vector<double> surf1, surf2;
    std::vector<int> idx;
    double E[9];
    std::vector<unsigned char> flags;
};
static std::vector<Entry> g_entries;
static KeyFrame* g_kf = 0;
static int g_lastCam[2] = {-1, -1}, g_nDetect = 0;
static const Entry* g_cur = 0;
struct Recorded {
    int called, gId1, gId2, iCam, jCam;
    std::vector<int> m;
};
static Recorded g_rec;

static void die(const char* what) {
    fprintf(stderr, "ref_mergematch_test: %s\n", what);
    exit(1);
}
int detectSURFPoints(const ImgG& img, Mat_d& surfPts, std::vector<float>& surfDesc) {
    int cam = -1;
    for (int c = 0; c < g_kf->nCam; ++c)
        if (&g_kf->pPose[c]->img == &img) cam = c;
    if (cam < 0) die("detectSURFPoints: not a key pose's image");
    g_lastCam[g_nDetect++ & 1] = cam;
    surfDesc.clear();
    g_cur = 0;
    if (!(g_nDetect & 1)) {   // the second of an entry's two calls: the entry is (first camera, this camera)
        for (size_t e = 0; e < g_entries.size(); ++e)
            if (g_entries[e].iCam == g_lastCam[0] && g_entries[e].jCam == g_lastCam[1]) g_cur = &g_entries[e];
        if (!g_cur) die("detectSURFPoints: no entry for this camera pair");
        const std::vector<double>& s = g_cur->surf2;
        surfPts.resize((int)s.size() / 2, 2);
        memcpy(surfPts.data, s.data(), s.size() * 8);
    } else {                  // the first: its list is the same for every entry that starts at this camera and names the same list
        const Entry* e0 = 0;
        for (size_t e = 0; e < g_entries.size() && !e0; ++e)
            if (g_entries[e].iCam == cam) e0 = &g_entries[e];
        if (!e0) die("detectSURFPoints: no entry starts at this camera");
        surfPts.resize((int)e0->surf1.size() / 2, 2);
        memcpy(surfPts.data, e0->surf1.data(), e0->surf1.size() * 8);
    }
    return 64;
}
int matchSurf(int, std::vector<float>&, std::vector<float>&, Matching& matches, double, double) {
    if (!g_cur) die("matchSurf outside an entry");
    matches.clear();
    for (int k = 0; k < g_cur->nMatch; ++k) matches.add(g_cur->idx[2 * k], g_cur->idx[2 * k + 1], 0);
    return matches.num;
}
int estimateEMat(const double*, const double*, const Mat_d&, const Mat_d&, const Matching&, double* E, int, double, int) {
    if (!g_cur) die("estimateEMat outside an entry");
    memcpy(E, g_cur->E, 72);
    return 1;
}
int evaluateEMat(int n, const double*, const double*, const double*, double, double& epiErr, unsigned char* inlierFlag) {
    if (!g_cur || n != g_cur->nMatch) die("evaluateEMat outside an entry");
    int cnt = 0;
    for (int k = 0; k < n; ++k) inlierFlag[k] = g_cur->flags[k], cnt += g_cur->flags[k] ? 1 : 0;
    epiErr = 0;
    return cnt;
}
bool refRecordGenMergeInfo(int gId1, int gId2, int iCam, int jCam, const Matching& featMatches) {
    g_rec.called = 1, g_rec.gId1 = gId1, g_rec.gId2 = gId2, g_rec.iCam = iCam, g_rec.jCam = jCam;
    g_rec.m.clear();
    for (int k = 0; k < featMatches.num; ++k) g_rec.m.push_back(featMatches[k].idx1), g_rec.m.push_back(featMatches[k].idx2);
    return true;
}

template <class T> static void get(FILE* f, T* p, size_t n) {
    if (n && fread(p, sizeof(T), n, f) != n) die("short input");
}
static int geti(FILE* f) {
    int v;
    get(f, &v, 1);
    return v;
}
template <class T> static void put(FILE* f, const T* p, size_t n) { fwrite(p, sizeof(T), n, f); }
static void puti(FILE* f, int v) { fwrite(&v, 4, 1, f); }

int main(int argc, char** argv) {
    if (argc < 4 || strcmp(argv[1], "golden")) {
        fprintf(stderr, "usage: %s golden <in.bin> <out.bin>\n", argv[0]);
        return 2;
    }
    FILE* in = fopen(argv[2], "rb");
    FILE* out = fopen(argv[3], "wb");
    if (!in || !out) return 1;
    const int nScenes = geti(in);
    for (int sc = 0; sc < nScenes; ++sc) {
        const int nC = geti(in), N = geti(in), Ws = geti(in), Hs = geti(in), frame = geti(in);
        double scale, par[3];   // par: maxEpiErr, minNcc, maxDisp of the driver's own calls (the loop's are the reference's 20.0, 0.45, 150)
        get(in, &scale, 1), get(in, par, 3);
        if (nC < 1 || nC > SLAM_MAX_NUM) die("the reference holds at most SLAM_MAX_NUM cameras");
        const int nGroup = geti(in);
        CameraGroup groups[SLAM_MAX_NUM];
        for (int g = 0; g < nGroup; ++g) {
            const int n = geti(in);
            for (int i = 0; i < n; ++i) groups[g].addCam(geti(in));
        }
        KeyFrame* kf = g_kf = new KeyFrame(frame);
        kf->setCamNum(nC);
        kf->setCamGroups(groups, nGroup);
        std::vector<std::vector<int> > slotOf(nC);
        for (int c = 0; c < nC; ++c) {
            double K[9];
            std::vector<double> xy(2 * (size_t)N);
            std::vector<int> state(N);
            get(in, K, 9), get(in, xy.data(), xy.size()), get(in, state.data(), state.size());
            ImgG small;
            small.resize(Ws, Hs);
            get(in, small.data, (size_t)Ws * Hs);
            CamPoseItem* cp = new CamPoseItem();
            cp->f = frame, cp->camId = c;
            KeyPose* kp = new KeyPose(frame, cp);
            kp->setCameraIntrinsic(K);
            kp->setSmallImage(small, scale);
            FeaturePoint *head = 0, *tail = 0;
            for (int s = 0; s < N; ++s) {
                if (state[s] != 0 && state[s] != 1) continue;
                FeaturePoint* fp = new FeaturePoint(frame, c, xy[s], xy[N + s]);
                fp->next = 0;
                if (tail) tail->next = fp;
                else head = fp;
                tail = fp;
                slotOf[c].push_back(s);
            }
            if (!head) die("a camera without a feature");
            kp->setFeatPoints(head, tail);
            kf->setKeyPose(c, kp);
        }
        MergeCameraGroup* mcg = new MergeCameraGroup();
        mcg->setCurrentFrame(kf);
        const int nInfo = geti(in);
        g_entries.assign(nInfo, Entry());
        double Z9[9] = {0}, Z3[9] = {0};
        mcg->m_nMergeInfo = 0;
        for (int e = 0; e < nInfo; ++e) {
            Entry& q = g_entries[e];
            q.iCam = geti(in), q.gId1 = geti(in), q.jCam = geti(in), q.gId2 = geti(in);
            const int n1 = geti(in);
            q.surf1.resize(2 * (size_t)n1), get(in, q.surf1.data(), q.surf1.size());
            const int n2 = geti(in);
            q.surf2.resize(2 * (size_t)n2), get(in, q.surf2.data(), q.surf2.size());
            q.nMatch = geti(in);
            q.idx.resize(2 * (size_t)q.nMatch), get(in, q.idx.data(), q.idx.size());
            get(in, q.E, 9);
            q.flags.resize(q.nMatch), get(in, q.flags.data(), q.flags.size());
            mcg->addMergeInfo(false, frame, q.iCam, q.gId1, frame, q.jCam, q.gId2, Z9, Z9, Z3);
        }
        mcg->storeFeaturePoints();
        for (int c = 0; c < nC; ++c)
            if (mcg->m_featPoints[c].size() != slotOf[c].size()) die("storeFeaturePoints: a list is not the live slots");
        // ---- every job on its own: the reference's matchFeaturePointsNCC ----
        for (int e = 0; e < nInfo; ++e) {
            const Entry& q = g_entries[e];
            int inl = 0;
            for (int k = 0; k < q.nMatch; ++k) inl += q.flags[k] ? 1 : 0;
            const int ran = q.nMatch >= 25 && inl >= 15;
            puti(out, ran);
            double iK1[9], iK2[9], Et[9], F[9];   // as :282-290
            mat33Inv(kf->pPose[q.iCam]->K, iK1), mat33Inv(kf->pPose[q.jCam]->K, iK2);
            mat33Trans(q.E, Et);
            getFMat(iK2, iK1, Et, F);
            put(out, F, 9);
            Matching newMatches, feat;
            if (ran) {
                for (int k = 0; k < q.nMatch; ++k)
                    if (q.flags[k]) newMatches.add(q.idx[2 * k], q.idx[2 * k + 1], 0);
                Mat_d s1((int)q.surf1.size() / 2, 2, q.surf1.data()), s2((int)q.surf2.size() / 2, 2, q.surf2.data());
                mcg->matchFeaturePointsNCC(q.iCam, q.jCam, mcg->m_featPoints[q.iCam], mcg->m_featPoints[q.jCam], s1, s2, newMatches, q.E, feat, par[0],
                                           par[1], par[2]);
            }
            puti(out, feat.num);
            for (int k = 0; k < feat.num; ++k) {   // list indices -> slots
                puti(out, slotOf[q.iCam][feat[k].idx1]), puti(out, slotOf[q.jCam][feat[k].idx2]);
                put(out, &feat[k].dist, 1);
            }
        }
        // ---- the loop ----
        g_rec = Recorded();
        g_nDetect = 0, g_cur = 0;
        mcg->m_gid1 = mcg->m_gid2 = mcg->m_camid1 = mcg->m_camid2 = -1;
        const int numMatched = mcg->matchMergableCameras();
        puti(out, numMatched), puti(out, g_rec.called);
        puti(out, g_rec.gId1), puti(out, g_rec.gId2), puti(out, g_rec.iCam), puti(out, g_rec.jCam);
        puti(out, mcg->m_gid1), puti(out, mcg->m_gid2), puti(out, mcg->m_camid1), puti(out, mcg->m_camid2);
        puti(out, (int)g_rec.m.size() / 2);
        for (size_t k = 0; k + 1 < g_rec.m.size(); k += 2)
            puti(out, slotOf[g_rec.iCam][g_rec.m[k]]), puti(out, slotOf[g_rec.jCam][g_rec.m[k + 1]]);
        printf("  scene %d: %d cameras x %d slots, %d entries -> numMatched %d, pair (%d, %d) of groups (%d, %d), %d matches\n", sc, nC, N, nInfo,
               numMatched, g_rec.iCam, g_rec.jCam, g_rec.gId1, g_rec.gId2, (int)g_rec.m.size() / 2);
    }
    fclose(in), fclose(out);
    printf("ref_mergematch_test: %d scenes\n", nScenes);
    return 0;
}
