// mergematch_front_shim_test.cpp -- CoSLAMMergeMatch::matchFeaturePointsNCCFront (include/shim/app/CoSLAMMergeMatch.h): the job's E, seed
// count and seed rows read from DEVICE memory in the layout of a cs_merge_front's buffers, against matchFeaturePointsNCC given the same E
// and seeds from the host -- the same Matching, bit for bit -- and a job the front gave up (too few SURF matches), which must come back
// empty with count.flags = CS_MERGE_MATCH_SKIPPED.  tests/test_mergematch_front_shim_gpu.py compiles it with g++ and writes <in.bin>
// (the format of mergematch_shim_test.cpp):
//   mergematch_front_shim_test <in.bin>
#include <hip/hip_runtime_api.h>

#include <cstdio>
#include <cstring>
#include <vector>

#include "app/CoSLAMMergeMatch.h"

#define HIPOK(x)                                          \
    do {                                                  \
        if ((x) != hipSuccess) {                          \
            fprintf(stderr, "HIP call failed: %s\n", #x); \
            return 3;                                     \
        }                                                 \
    } while (0)

template <class T> static bool rd(FILE* f, T* p, size_t n) { return fread(p, sizeof(T), n, f) == n; }
template <class T> static T* up(const std::vector<T>& v) {
    T* d = 0;
    if (hipMalloc((void**)&d, v.size() * sizeof(T) + 8) != hipSuccess) return 0;
    if (!v.empty() && hipMemcpy(d, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice) != hipSuccess) return 0;
    return d;
}
struct Mat_d {   // the members of the reference's Mat_d that getMatchedPts reads
    int rows, cols;
    std::vector<double> store;
    double* data;
};
struct Match {
    int idx1, idx2;
    double dist;
};
struct Matching {   // the members of the reference's Matching on this path
    int num;
    std::vector<Match> data;
    Matching() : num(0) {}
    void clear() { data.clear(), num = 0; }
    void add(int i1, int i2, double d) {
        Match m = {i1, i2, d};
        data.push_back(m), num = (int)data.size();
    }
    const Match& operator[](int i) const { return data[i]; }
};

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    int nC, N, Ws, Hs;
    double scale;
    if (!rd(f, &nC, 1) || !rd(f, &N, 1) || !rd(f, &Ws, 1) || !rd(f, &Hs, 1) || !rd(f, &scale, 1)) return 2;
    std::vector<std::vector<double> > K(nC, std::vector<double>(9)), xy(nC, std::vector<double>(2 * (size_t)N));
    std::vector<std::vector<int> > state(nC, std::vector<int>(N));
    std::vector<std::vector<unsigned char> > img(nC, std::vector<unsigned char>((size_t)Ws * Hs));
    try {
        CoSLAMMergeMatch matcher(nC, N, 64, 1 << 16, N);
        matcher.setSmallImageSize(Ws, Hs);
        for (int c = 0; c < nC; ++c) {
            if (!rd(f, K[c].data(), 9) || !rd(f, xy[c].data(), 2 * (size_t)N) || !rd(f, state[c].data(), N) || !rd(f, img[c].data(), img[c].size())) return 2;
            cs_merge_match_cam cam;
            cam.xy = up(xy[c]), cam.state = up(state[c]), cam.K = K[c].data(), cam.imgSmall = up(img[c]), cam.imgScale = scale;
            if (!cam.xy || !cam.state || !cam.imgSmall) return 3;
            matcher.setCamera(c, cam);
            matcher.storeFeaturePoints(c, state[c].data());
        }
        int iCam, jCam, nM;
        double E[9];
        Mat_d s[2];
        if (!rd(f, &iCam, 1) || !rd(f, &jCam, 1) || !rd(f, E, 9)) return 2;
        for (int q = 0; q < 2; ++q) {
            if (!rd(f, &s[q].rows, 1)) return 2;
            s[q].cols = 2, s[q].store.resize(2 * (size_t)s[q].rows + 2), s[q].data = s[q].store.data();
            if (!rd(f, s[q].data, 2 * (size_t)s[q].rows)) return 2;
        }
        if (!rd(f, &nM, 1)) return 2;
        Matching surf, feat;
        for (int k = 0; k < nM; ++k) {
            int ab[2];
            if (!rd(f, ab, 2)) return 2;
            surf.add(ab[0], ab[1], 0);
        }
        fclose(f);
        const int n = matcher.matchFeaturePointsNCC(iCam, jCam, s[0], s[1], surf, E, feat, 20.0, 0.45, 150);
        if (n != feat.num || n < 10) return 4;
        // the same job as a cs_merge_front leaves it: one result record, the inliers' rows {x1, y1, x2, y2} in a block of seedRows rows
        const int seedRows = nM + 7;
        std::vector<cs_merge_front_result> res(2);
        memset(res.data(), 0, sizeof(cs_merge_front_result) * 2);
        std::vector<double> rows(2 * 4 * (size_t)seedRows, 0.0);
        for (int q = 0; q < 2; ++q) {
            res[q].surfNum = q == 0 ? nM + 20 : 24, res[q].ematOk = 1, res[q].inlierNum = nM;   // job 1: one SURF match short of 25
            for (int k = 0; k < 9; ++k) res[q].E[k] = E[k];
            for (int k = 0; k < nM; ++k) {
                double* r = &rows[4 * ((size_t)q * seedRows + k)];
                r[0] = s[0].data[2 * surf[k].idx1], r[1] = s[0].data[2 * surf[k].idx1 + 1];
                r[2] = s[1].data[2 * surf[k].idx2], r[3] = s[1].data[2 * surf[k].idx2 + 1];
            }
        }
        const cs_merge_front_result* d_res = up(res);
        const double* d_rows = up(rows);
        if (!d_res || !d_rows) return 3;
        Matching got, none;
        const int m = matcher.matchFeaturePointsNCCFront(iCam, jCam, d_res, d_rows, seedRows, got, 20.0, 0.45, 150);
        if (m != n || got.num != n || matcher.count.flags != 0) return 5;
        for (int k = 0; k < n; ++k)
            if (got[k].idx1 != feat[k].idx1 || got[k].idx2 != feat[k].idx2 || memcmp(&got[k].dist, &feat[k].dist, sizeof(double)) != 0) return 6;
        none.add(1, 2, 3.0);
        const int z = matcher.matchFeaturePointsNCCFront(iCam, jCam, d_res + 1, d_rows + 4 * (size_t)seedRows, seedRows, none, 20.0, 0.45, 150);
        if (z != 0 || none.num != 0 || matcher.count.flags != CS_MERGE_MATCH_SKIPPED || matcher.count.count != 0) return 7;
    } catch (const std::exception& e) {
        fprintf(stderr, "%s\n", e.what());
        return 1;
    }
    printf("shim ok\n");
    return 0;
}
