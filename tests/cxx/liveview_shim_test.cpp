// liveview_shim_test.cpp -- include/shim/app/CoSLAMLiveView.h over a planted six-frame sequence: what the shim's storeDynamicPoints leaves in
// m_dynPts frame by frame and what its getDynTracks gives at the end, printed as one JSON line for tests/test_liveview_gpu.py, which holds
// it against the restatement (tests/liveview_ref.py: trail_sequence() is this file's sequence).  A local stand-in for LibVisualSLAM's
// Point3dId; no reference headers.  Built by __graft_entry__.build() into tests/cxx/liveview_shim_test.bin.
//
// The sequence (2 cameras, 8 map rows, point r of frame f at (r + 0.25 f, 10 r - f, 0.5 r f)): row 0 static throughout; A = row 1 dynamic
// throughout; B = row 3 dynamic, without a feature at frame 4, back at frame 5; C = row 4 dynamic up to frame 3, static from frame 4;
// D = row 6 first seen (dynamic) at frame 5.  trailDepth = 4, so the ring wraps.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "app/CoSLAMLiveView.h"

struct Point3dId {   // stand-in: LibVisualSLAM's is (x, y, z, id)
    double x, y, z;
    size_t id;
    Point3dId(double x_, double y_, double z_, size_t id_) : x(x_), y(y_), z(z_), id(id_) {}
};

#define HIPCHK(x)                                                                          \
    do {                                                                                   \
        hipError_t e_ = (x);                                                               \
        if (e_ != hipSuccess) {                                                            \
            fprintf(stderr, "%s: %s (%s:%d)\n", #x, hipGetErrorString(e_), __FILE__, __LINE__); \
            exit(3);                                                                       \
        }                                                                                  \
    } while (0)

static std::string json(const std::vector<std::vector<Point3dId> >& v) {
    std::string s = "[";
    char buf[160];
    for (size_t a = 0; a < v.size(); ++a) {
        s += a ? ", [" : "[";
        for (size_t b = 0; b < v[a].size(); ++b) {
            const Point3dId& p = v[a][b];
            snprintf(buf, sizeof(buf), "%s[%zu, %.17g, %.17g, %.17g]", b ? ", " : "", p.id, p.x, p.y, p.z);
            s += buf;
        }
        s += "]";
    }
    return s + "]";
}

int main() {
    const int nC = 2, nMap = 8, T = 6;
    int* dPf;
    unsigned char* dFlags;
    double *dPts, *dR, *dT;
    int* dCount;
    HIPCHK(hipSetDevice(0));
    HIPCHK(hipMalloc((void**)&dPf, sizeof(int) * nMap * nC));
    HIPCHK(hipMalloc((void**)&dFlags, nMap));
    HIPCHK(hipMalloc((void**)&dPts, sizeof(double) * 3 * nMap));
    HIPCHK(hipMalloc((void**)&dR, sizeof(double) * 9 * nC));
    HIPCHK(hipMalloc((void**)&dT, sizeof(double) * 3 * nC));
    HIPCHK(hipMalloc((void**)&dCount, sizeof(int)));
    HIPCHK(hipMemset(dR, 0, sizeof(double) * 9 * nC));
    HIPCHK(hipMemset(dT, 0, sizeof(double) * 3 * nC));
    HIPCHK(hipMemcpy(dCount, &nMap, sizeof(int), hipMemcpyHostToDevice));
    hipStream_t s;
    HIPCHK(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));

    std::vector<std::vector<Point3dId> > m_dynPts, dynTracks, tracks3;
    int nStatic = -1, nDynamic = -1, nSF[2] = {-1, -1}, nDF[2] = {-1, -1};
    try {
        CoSLAMLiveView<Point3dId> live(nC, /*curCap*/ 8, /*dynCap*/ 8, /*depth*/ 2, /*trailDepth*/ 4, /*every*/ 1);
        for (int f = 0; f < T; ++f) {
            std::vector<int> pf(nMap * nC, -1);
            std::vector<unsigned char> fl(nMap, 0);
            std::vector<double> pts(3 * nMap);
            for (int r = 0; r < nMap; ++r) pts[3 * r] = r + 0.25 * f, pts[3 * r + 1] = 10.0 * r - f, pts[3 * r + 2] = 0.5 * r * f;
            auto seen = [&](int r, int c) { pf[r * nC + c] = 10 * r + c; };
            seen(0, 0), seen(0, 1);
            seen(1, 0), seen(1, 1), fl[1] = CS_MAP_DYNAMIC;
            fl[3] = CS_MAP_DYNAMIC;
            if (f != 4) seen(3, 1);
            seen(4, 0), fl[4] = f <= 3 ? CS_MAP_DYNAMIC : 0;
            fl[6] = CS_MAP_DYNAMIC;
            if (f == 5) seen(6, 0), seen(6, 1);
            HIPCHK(hipMemcpyAsync(dPf, pf.data(), sizeof(int) * nMap * nC, hipMemcpyHostToDevice, s));
            HIPCHK(hipMemcpyAsync(dFlags, fl.data(), nMap, hipMemcpyHostToDevice, s));
            HIPCHK(hipMemcpyAsync(dPts, pts.data(), sizeof(double) * 3 * nMap, hipMemcpyHostToDevice, s));
            live.frame((void*)s, f, nMap, dCount, dPf, dFlags, dPts, dR, dT);
            HIPCHK(hipStreamSynchronize(s));   // (the test's wait: the frame has landed, so storeDynamicPoints appends it)
            if (!live.storeDynamicPoints(m_dynPts)) {
                fprintf(stderr, "frame %d: storeDynamicPoints appended nothing although the frame has landed\n", f);
                return 4;
            }
            if (live.storeDynamicPoints(m_dynPts)) {
                fprintf(stderr, "frame %d: storeDynamicPoints appended the same frame twice\n", f);
                return 4;
            }
        }
        live.getDynTracks((void*)s, dynTracks, 4);
        live.getDynTracks((void*)s, tracks3, 3);
        if (!live.numDynamicStaticPoints(nStatic, nDynamic, nSF, nDF, nC)) return 4;
    } catch (const std::exception& ex) {
        fprintf(stderr, "%s\n", ex.what());
        return 3;
    }
    printf("{\"m_dynPts\": %s, \"dynTracks\": %s, \"dynTracks3\": %s, \"nStatic\": %d, \"nDynamic\": %d, \"nStaticFeat\": [%d, %d], "
           "\"nDynamicFeat\": [%d, %d]}\n",
           json(m_dynPts).c_str(), json(dynTracks).c_str(), json(tracks3).c_str(), nStatic, nDynamic, nSF[0], nSF[1], nDF[0], nDF[1]);
    return 0;
}
