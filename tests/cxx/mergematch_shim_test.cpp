// mergematch_shim_test.cpp -- include/shim/app/CoSLAMMergeMatch.h driven the way MergeCameraGroup::matchMergableCameras would (reference
// src/app/SL_MergeCameraGroup.cpp:381-383): the current key frame's positions, states and small images are put into device memory, the
// features stored, the SURF positions and the E matrix' inlier matches handed over as the reference's Mat_d / Matching, and
// matchFeaturePointsNCC fills a Matching with LIST indices.  tests/test_mergematch_shim_gpu.py compiles it with g++, writes <in.bin> and
// compares <out.bin> with the restatement tests/mergematch_ref.py:
//   mergematch_shim_test <in.bin> <out.bin>
// in:  int nC, N, Ws, Hs; double scale; per camera K[9], xy[2N], int state[N], unsigned char img[Ws Hs];
//      int iCam, jCam; double E[9]; int n1; double surf1[n1][2]; int n2; double surf2[n2][2]; int nM; int idx[nM][2]
// out: int n, flags, candidates, rounds; per match int idx1, idx2, double score; then the n SLOT pairs of matches_ptr()
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
    if (argc < 3) return 2;
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
        if (n != feat.num) return 4;
        std::vector<int> slots(2 * (size_t)n + 2);
        HIPOK(hipMemcpy(slots.data(), matcher.matches_ptr(), 8 * (size_t)n, hipMemcpyDeviceToHost));
        FILE* o = fopen(argv[2], "wb");
        if (!o) return 2;
        fwrite(&matcher.count, sizeof(int), 4, o);
        for (int k = 0; k < n; ++k) fwrite(&feat[k].idx1, sizeof(int), 1, o), fwrite(&feat[k].idx2, sizeof(int), 1, o), fwrite(&feat[k].dist, sizeof(double), 1, o);
        fwrite(slots.data(), sizeof(int), 2 * (size_t)n, o);
        fclose(o);
    } catch (const std::exception& e) {
        fprintf(stderr, "%s\n", e.what());
        return 1;
    }
    printf("shim ok\n");
    return 0;
}
