// include/shim/app/CoSLAMMergeFront.h driven with reference-shaped arguments (Mat_d, vector<float>, Matching) on a scene read from a file
// (tests/test_mergefront_shim_gpu.py writes it and checks what comes back against the numpy restatement).
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "app/CoSLAMMergeFront.h"

struct Mat_d {   // the reference's Mat_d as far as the shim reads it
    int rows, cols;
    double* data;
};
struct MatchItem {
    int idx1, idx2;
    double dist;
};
struct Matching {   // the reference's Matching as far as the shim uses it
    int num;
    std::vector<MatchItem> v;
    Matching() : num(0) {}
    void clear() { v.clear(), num = 0; }
    void add(int a, int b, double d) {
        MatchItem m = {a, b, d};
        v.push_back(m), num = (int)v.size();
    }
    const MatchItem& operator[](int k) const { return v[k]; }
};

template <class T>
static bool rd(FILE* f, T* p, size_t n) { return fread(p, sizeof(T), n, f) == n; }

int main(int argc, char** argv) {
    if (argc < 3) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    int hdr[6];   // nCams, iCam, jCam, dim, nRansac, minInlierNum
    unsigned long long seed;
    double K[9];
    int n1, n2;
    if (!rd(f, hdr, 6) || !rd(f, &seed, 1) || !rd(f, K, 9) || !rd(f, &n1, 1) || !rd(f, &n2, 1)) return 3;
    const int dim = hdr[3];
    std::vector<double> p1(2 * (size_t)n1), p2(2 * (size_t)n2);
    std::vector<float> d1((size_t)n1 * dim), d2((size_t)n2 * dim);
    if (!rd(f, p1.data(), p1.size()) || !rd(f, p2.data(), p2.size()) || !rd(f, d1.data(), d1.size()) || !rd(f, d2.data(), d2.size())) return 3;
    fclose(f);
    Mat_d m1 = {n1, 2, p1.data()}, m2 = {n2, 2, p2.data()};
    try {
        CoSLAMMergeFront front(hdr[0], n1 > n2 ? n1 : n2, dim, hdr[4]);
        front.seed = seed;
        for (int c = 0; c < hdr[0]; ++c) front.setK(c, K);
        Matching matches, newMatches;
        double E[9];
        const int n = front.matchSURFPoints(hdr[1], hdr[2], m1, m2, dim, d1, d2, matches);
        const int m = front.computeEMat(hdr[1], hdr[2], m1, m2, matches, newMatches, E, hdr[4], 2.0, hdr[5]);
        FILE* o = fopen(argv[2], "wb");
        if (!o) return 2;
        fwrite(&n, 4, 1, o), fwrite(&m, 4, 1, o);
        for (int k = 0; k < n; ++k) fwrite(&matches.v[k], sizeof(MatchItem), 1, o);
        fwrite(E, 8, 9, o);
        fwrite(&front.result, sizeof(front.result), 1, o);
        for (int k = 0; k < newMatches.num; ++k) fwrite(&newMatches.v[k], sizeof(MatchItem), 1, o);
        fwrite(front.seeds().data(), 8, front.seeds().size(), o);
        fclose(o);
        // a pair below minInlierNum: 0, newMatches untouched
        Matching keep = newMatches;
        const int z = front.computeEMat(hdr[1], hdr[2], m1, m2, matches, newMatches, E, hdr[4], 2.0, n + 1);
        if (z != 0 || newMatches.num != keep.num) {
            printf("computeEMat below minInlierNum: %d, %d matches\n", z, newMatches.num);
            return 4;
        }
    } catch (const std::exception& e) {
        printf("exception: %s\n", e.what());
        return 5;
    }
    printf("shim ok\n");
    return 0;
}
