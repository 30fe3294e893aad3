// ref_mergegraph_test.cpp -- the reference's OWN GlobalPoseGraph::computeNewCameraRotations + computeNewCameraTranslations4
// (src/slam/SL_GlobalPoseEstimation.cpp:52-219, 361-525) on merge-shaped key-frame graphs: the fixture that pins the
// uncertain-scale half of the pose-graph relaxation (cs_posegraph_create_scaled / cs_posegraph_relax_scaled).
//
// The graphs are built with the reference's classes the way MergeCameraGroup::_constructGraphForKeyFrms does
// (src/app/SL_MergeCameraGroup.cpp:907-1035): nodes frame-major over the cameras, the oldest key frame fixed; per key frame
// up to the first-constrained one the chain over every camera group (plus the closing edge of a group of more than two),
// then the successive-frame edges; the constraint edges last (scale id 0, uncertainScale, constraint, the nodes' constraint
// flag, nFixedNode, nConstraintEdge).  Four hand-made graphs cover what CoSLAM never builds: two scale ids, one scale
// shared by two components that fixed nodes separate, uncertain-scale edges whose id2 is fixed (with a fixed-fixed one,
// which gives no equation but still receives the scale, :515-522), and uncertain-scale edges whose id1 is fixed.
// The last one cannot go through the reference as it stands: for that case :495 calls mat33AB -- the 3x3 * 3x3 product -- on
// the fixed node's 3-vector t, which reads six doubles past t and writes nine right-hand-side entries instead of three (past
// the end of b for the last rows).  That is a defect, not behaviour; CoSLAM never reaches it (a constraint edge never ends in
// the fixed frame).  What the branch means is b = R_ij T_i.  The driver therefore hands the reference the MIRRORED edge
// (j -> i, R^T, -R^T t: the same equations multiplied by the orthogonal -R^T, so the same least-squares solution, now through
// the well-defined id2-fixed branch) and writes the graph with the edge as given.
//   ref_mergegraph_test golden <out.bin>    CPU only.  tests/golden/make_mergegraph_golden.py turns the file into
//                                            tests/golden/mergegraph_golden.npz.
// Built by oracle/Makefile, target _ref/ref_mergegraph_test (where the reference tree exists).
// Sparse QR, the polar factor and mat33* are un-vendored LibVisualSLAM: the stand-ins of ref_shim/ref_posegraph_impl.cpp.
// TEST INFRASTRUCTURE; the binary goes to oracle/_ref/ (untracked), nothing on the GPU side needs it.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "geometry/SL_RigidTransform.h"
#include "math/SL_LinAlg.h"
#include "slam/SL_GlobalPoseEstimation.h"

static unsigned long long g_rng = 0x9E3779B97F4A7C15ull;
static double urand() {
    g_rng ^= g_rng << 13;
    g_rng ^= g_rng >> 7;
    g_rng ^= g_rng << 17;
    return (double)(g_rng >> 11) / 9007199254740992.0;
}
static double srand1() { return 2 * urand() - 1; }

static void rodrigues(const double w[3], double R[9]) {
    const double th = sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2]);
    const double k[3] = {th > 0 ? w[0] / th : 1, th > 0 ? w[1] / th : 0, th > 0 ? w[2] / th : 0};
    const double c = cos(th), s = sin(th), v = 1 - c;
    R[0] = c + k[0] * k[0] * v, R[1] = k[0] * k[1] * v - k[2] * s, R[2] = k[0] * k[2] * v + k[1] * s;
    R[3] = k[1] * k[0] * v + k[2] * s, R[4] = c + k[1] * k[1] * v, R[5] = k[1] * k[2] * v - k[0] * s;
    R[6] = k[2] * k[0] * v - k[1] * s, R[7] = k[2] * k[1] * v + k[0] * s, R[8] = c + k[2] * k[2] * v;
}

struct Pose {
    double R[9], t[3];
};

// a smooth trajectory of n key frames (a key frame every few dozen frames: larger steps than frame to frame)
static std::vector<Pose> trajectory(int n) {
    std::vector<Pose> tr(n);
    double w[3] = {0.3 * srand1(), 0.3 * srand1(), 0.3 * srand1()}, p[3] = {2 * srand1(), 2 * srand1(), 4 + srand1()};
    double dw[3] = {0.05 * srand1(), 0.05 * srand1(), 0.05 * srand1()}, dp[3] = {0.3 * srand1(), 0.3 * srand1(), 0.3 * srand1()};
    for (int i = 0; i < n; ++i) {
        rodrigues(w, tr[i].R);
        memcpy(tr[i].t, p, sizeof(p));
        for (int q = 0; q < 3; ++q) {
            dw[q] += 0.01 * srand1();
            dp[q] += 0.05 * srand1();
            w[q] += dw[q];
            p[q] += dp[q];
        }
    }
    return tr;
}

// the true trajectory with a drift that grows from frame `from` on: what tracking without the other group's points leaves
static std::vector<Pose> drifted(const std::vector<Pose>& tr, int from, double rot, double trans) {
    std::vector<Pose> out(tr);
    double w[3] = {0, 0, 0}, d[3] = {0, 0, 0};
    for (size_t i = 0; i < tr.size(); ++i) {
        if ((int)i > from)
            for (int q = 0; q < 3; ++q) w[q] += rot * srand1(), d[q] += trans * (0.5 + urand());
        double dR[9];
        rodrigues(w, dR);
        mat33AB(dR, tr[i].R, out[i].R);
        for (int q = 0; q < 3; ++q) out[i].t[q] = tr[i].t[q] + d[q];
    }
    return out;
}

static void plain_edge(GlobalPoseGraph& g, const Pose& a, const Pose& b, int i, int j) {
    double R[9], t[3];
    getRigidTransFromTo(a.R, a.t, b.R, b.t, R, t);
    g.addEdge()->set(i, j, R, t);
}

// MergeInfo::R / t: the relative pose of the TRUE poses, the translation known up to `scale`, a little measurement noise
static void constraint_edge(GlobalPoseGraph& g, const Pose& a, const Pose& b, int i, int j, int sid, double scale, double noise) {
    double R[9], t[3];
    getRigidTransFromTo(a.R, a.t, b.R, b.t, R, t);
    const double w[3] = {noise * srand1(), noise * srand1(), noise * srand1()};
    double dR[9], R2[9];
    rodrigues(w, dR);
    mat33AB(dR, R, R2);
    for (int q = 0; q < 3; ++q) t[q] = scale * (t[q] + noise * srand1());
    CamPoseEdge* e = g.addEdge();
    e->set(i, j, R2, t, sid);
    e->uncertainScale = true;
    e->constraint = true;
    g.poseNodes[i].constraint = true;
    g.poseNodes[j].constraint = true;
    g.nConstraintEdge++;
}

// nC cameras x nK key frames; cameras [0, split) and [split, nC) are two groups from frame 1 on (one group in frame 0, the
// fixed frame); F = the first-constrained key frame; the second group drifts after F; the constraint edges join frame F's
// cameras of the first group to the current (last) frame's cameras of the second group, and the two groups' first cameras
// in the current frame
static void build_merge_graph(GlobalPoseGraph& g, int nC, int nK, int F, int split, double scale) {
    std::vector<std::vector<Pose> > truth(nC), cur(nC);
    for (int c = 0; c < nC; ++c) {
        truth[c] = trajectory(nK);
        cur[c] = c >= split ? drifted(truth[c], F, 0.01, 0.05) : truth[c];
    }
    g.reserve(nC * nK, 3 * nC * nK);
    g.nFixedNode = 0;
    for (int f = 0; f < nK; ++f)
        for (int c = 0; c < nC; ++c) {
            CamPoseNode* nd = g.newNode();
            nd->set(10 * f, c, cur[c][f].R, cur[c][f].t);
            nd->fixed = f == 0;
            if (nd->fixed) g.nFixedNode++;
        }
    for (int f = 0; f < nK; ++f) {
        std::vector<std::vector<int> > groups;
        if (f == 0) {
            groups.resize(1);
            for (int c = 0; c < nC; ++c) groups[0].push_back(c);
        } else {
            groups.resize(2);
            for (int c = 0; c < nC; ++c) groups[c >= split].push_back(c);
        }
        for (size_t q = 0; q < groups.size(); ++q) {
            const std::vector<int>& ids = groups[q];
            if (ids.size() > 1 && f <= F) {
                size_t i = 1;
                for (; i < ids.size(); ++i) plain_edge(g, cur[ids[i - 1]][f], cur[ids[i]][f], f * nC + ids[i - 1], f * nC + ids[i]);
                if (ids.size() > 2) plain_edge(g, cur[ids[i - 1]][f], cur[ids[0]][f], f * nC + ids[i - 1], f * nC + ids[0]);
            }
        }
        if (f > 0)
            for (int c = 0; c < nC; ++c) plain_edge(g, cur[c][f - 1], cur[c][f], (f - 1) * nC + c, f * nC + c);
    }
    g.nConstraintEdge = 0;
    const int L = nK - 1;
    for (int i = 0; i < split && split + i < nC; ++i)
        constraint_edge(g, truth[i][F], truth[split + i][L], F * nC + i, L * nC + split + i, 0, scale, 0.002);
    constraint_edge(g, truth[0][L], truth[split][L], L * nC + 0, L * nC + split, 0, scale, 0.002);
    if (nC - split > 1) constraint_edge(g, truth[0][F], truth[nC - 1][L], F * nC + 0, L * nC + nC - 1, 0, scale, 0.002);
}

// a chain of n nodes with the given fixed nodes and constraint edges {id1, id2, scale id}
static void build_chain_graph(GlobalPoseGraph& g, int n, const std::vector<int>& fixedList, const std::vector<std::vector<int> >& cons,
                              const double* scales) {
    const std::vector<Pose> truth = trajectory(n), cur = drifted(truth, 0, 0.005, 0.03);
    g.reserve(n, 3 * n);
    g.nFixedNode = 0;
    for (int i = 0; i < n; ++i) g.newNode()->set(i, 0, cur[i].R, cur[i].t);
    for (size_t k = 0; k < fixedList.size(); ++k) {
        CamPoseNode& nd = g.poseNodes[fixedList[k]];
        nd.fixed = true;
        nd.set(truth[fixedList[k]].R, truth[fixedList[k]].t);
        g.nFixedNode++;
    }
    for (int i = 1; i < n; ++i) plain_edge(g, cur[i - 1], cur[i], i - 1, i);
    g.nConstraintEdge = 0;
    for (size_t k = 0; k < cons.size(); ++k)
        constraint_edge(g, truth[cons[k][0]], truth[cons[k][1]], cons[k][0], cons[k][1], cons[k][2], scales[cons[k][2]], 0.002);
}

static const int N_GRAPHS = 9;
static void build_graph(GlobalPoseGraph& g, int which) {
    const double sc[4] = {0.4, 1.0, 1.0, 2.5};
    switch (which) {
    case 0: build_merge_graph(g, 2, 3, 1, 1, 0.37); break;     // one free frame between the fixed and the current frame
    case 1: build_merge_graph(g, 3, 4, 2, 1, 1.9); break;      // the closing group edge (3 cameras in one group)
    case 2: build_merge_graph(g, 8, 6, 3, 4, 0.6); break;
    case 3: build_merge_graph(g, 16, 4, 2, 8, 3.0); break;
    case 4: build_merge_graph(g, 8, 24, 15, 4, 0.25); break;   // leaves the LDS budget
    case 5: build_chain_graph(g, 10, {0}, {{2, 7, 0}, {3, 8, 0}, {1, 6, 3}, {4, 9, 3}}, sc); break;  // two scale ids (0 and 3)
    case 6: build_chain_graph(g, 9, {0, 4, 8}, {{1, 3, 0}, {5, 7, 0}}, sc); break;  // one scale, two components
    case 7: build_chain_graph(g, 8, {0, 7}, {{4, 7, 0}, {0, 7, 0}, {2, 5, 0}}, sc); break;  // id2 fixed, both fixed
    default: build_chain_graph(g, 8, {0, 7}, {{0, 3, 0}, {7, 5, 0}, {2, 4, 0}}, sc); break;  // id1 fixed
    }
}

// an uncertain-scale edge with id1 fixed and id2 free <-> its mirror image (see the header)
static int mirror_fixed_id1_edges(GlobalPoseGraph& g, const std::vector<int>* only, std::vector<int>* done) {
    int n = 0;
    for (int k = 0; k < g.nEdges; ++k) {
        CamPoseEdge& e = g.poseEdges[k];
        bool take = only ? false : (e.uncertainScale && g.poseNodes[e.id1].fixed && !g.poseNodes[e.id2].fixed);
        if (only)
            for (size_t q = 0; q < only->size(); ++q) take = take || (*only)[q] == k;
        if (!take) continue;
        double Rt[9], t[3];
        for (int r = 0; r < 3; ++r)
            for (int c = 0; c < 3; ++c) Rt[3 * r + c] = e.R[3 * c + r];
        for (int r = 0; r < 3; ++r) t[r] = -(Rt[3 * r] * e.t[0] + Rt[3 * r + 1] * e.t[1] + Rt[3 * r + 2] * e.t[2]);
        const int a = e.id1;
        e.id1 = e.id2, e.id2 = a;
        memcpy(e.R, Rt, sizeof(Rt));
        memcpy(e.t, t, sizeof(t));
        if (done) done->push_back(k);
        ++n;
    }
    return n;
}

static void write_graph(FILE* f, const GlobalPoseGraph& g) {
    const int hdr[4] = {g.nNodes, g.nEdges, g.nFixedNode, g.nConstraintEdge};
    fwrite(hdr, sizeof(int), 4, f);
    for (int i = 0; i < g.nNodes; ++i) {
        const CamPoseNode& nd = g.poseNodes[i];
        const int v[4] = {nd.fixed ? 1 : 0, nd.constraint ? 1 : 0, nd.frame, nd.camId};
        fwrite(v, sizeof(int), 4, f);
        fwrite(nd.R, sizeof(double), 9, f);
        fwrite(nd.t, sizeof(double), 3, f);
        fwrite(nd.newR, sizeof(double), 9, f);
        fwrite(nd.newt, sizeof(double), 3, f);
    }
    for (int k = 0; k < g.nEdges; ++k) {
        const CamPoseEdge& e = g.poseEdges[k];
        const int v[4] = {e.id1, e.id2, e.uncertainScale ? e.scaleId : -1, e.constraint ? 1 : 0};
        fwrite(v, sizeof(int), 4, f);
        fwrite(e.R, sizeof(double), 9, f);
        fwrite(e.t, sizeof(double), 3, f);
        fwrite(&e.s, sizeof(double), 1, f);
    }
}

int main(int argc, char** argv) {
    if (argc < 3 || strcmp(argv[1], "golden")) {
        fprintf(stderr, "usage: %s golden <out.bin>\n", argv[0]);
        return 2;
    }
    FILE* f = fopen(argv[2], "wb");
    if (!f) return 2;
    const int hdr[2] = {N_GRAPHS, 0};
    fwrite(hdr, sizeof(int), 2, f);
    for (int w = 0; w < N_GRAPHS; ++w) {
        GlobalPoseGraph g;
        build_graph(g, w);
        std::vector<int> mirrored;
        const int nm = mirror_fixed_id1_edges(g, 0, &mirrored);
        if ((w == N_GRAPHS - 1) != (nm > 0)) return 3;  // only the last graph has such edges
        g.computeNewCameraRotations();
        g.computeNewCameraTranslations4();
        if (nm) mirror_fixed_id1_edges(g, &mirrored, 0);  // back to the edges as given (twice mirrored = the original values up to rounding)
        write_graph(f, g);
        double s = 0;
        for (int k = 0; k < g.nEdges; ++k)
            if (g.poseEdges[k].uncertainScale) s = g.poseEdges[k].s;
        printf("  graph %d: %3d nodes %3d edges (%d constraint), scale of the last constraint edge %.6f\n", w, g.nNodes, g.nEdges,
               g.nConstraintEdge, s);
    }
    fclose(f);
    printf("ref_mergegraph_test: wrote %d graphs\n", N_GRAPHS);
    return 0;
}
