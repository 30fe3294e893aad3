// include/shim/app/CoSLAMSurf.h driven with reference-shaped arguments (ImgG, Mat_d, vector<float>) on an image read from a file
// (tests/test_surf_shim_gpu.py writes it and checks what comes back against coslam_amd.Surf).
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "app/CoSLAMSurf.h"

struct ImgG {   // the reference's ImgG as far as the shim reads it
    int rows, cols;
    unsigned char* data;
};
struct Mat_d {   // the reference's Mat_d as far as the shim uses it
    int rows, cols;
    double* data;
    Mat_d() : rows(0), cols(0), data(0) {}
    ~Mat_d() { delete[] data; }
    void resize(int r, int c) {
        delete[] data;
        rows = r, cols = c, data = new double[(size_t)(r * c > 0 ? r * c : 1)];
    }
};

static void put(FILE* o, const Mat_d& pts, const std::vector<float>& desc, int dim) {
    fwrite(&pts.rows, 4, 1, o), fwrite(&dim, 4, 1, o);
    fwrite(pts.data, 8, 2 * (size_t)pts.rows, o), fwrite(desc.data(), 4, desc.size(), o);
}

int main(int argc, char** argv) {
    if (argc < 3) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    int hdr[2];   // W, H
    double thr;
    if (fread(hdr, 4, 2, f) != 2 || fread(&thr, 8, 1, f) != 1) return 3;
    std::vector<unsigned char> px((size_t)hdr[0] * hdr[1]);
    if (fread(px.data(), 1, px.size(), f) != px.size()) return 3;
    fclose(f);
    ImgG img = {hdr[1], hdr[0], px.data()};
    try {
        FILE* o = fopen(argv[2], "wb");
        if (!o) return 2;
        Mat_d pts;
        std::vector<float> desc;
        coslamSurfOptions().hessianThreshold = thr, coslamSurfOptions().maxPts = 512;
        int dim = detectSURFPoints(img, pts, desc);                  // the reference's call; twice: the second goes to the cached handle
        dim = detectSURFPoints(img, pts, desc);
        if (dim != 64 || pts.cols != 2 || desc.size() != (size_t)pts.rows * dim) return 4;
        put(o, pts, desc, dim);
        cs_surf* own = cs_surf_create(0, 1, hdr[0], hdr[1], 512, 4, 2, 128);   // a caller-held handle: extended descriptors, upright
        if (!own) return 5;
        dim = detectSURFPoints(own, img, pts, desc, thr, 1);
        if (dim != 128 || desc.size() != (size_t)pts.rows * dim) return 4;
        put(o, pts, desc, dim);
        cs_surf_destroy(own);
        fclose(o);
    } catch (const std::exception& e) {
        printf("exception: %s\n", e.what());
        return 6;
    }
    printf("shim ok\n");
    return 0;
}
