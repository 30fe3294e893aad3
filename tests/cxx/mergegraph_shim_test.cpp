// mergegraph_shim_test.cpp -- include/shim/slam/coslam_posegraph.h's relaxScaledPoseGraph over a test-local graph type with
// the members the template binds to (SL_GlobalPoseEstimation.h:13-82).  tests/test_mergegraph_gpu.py compiles it with g++,
// writes a graph from tests/golden/mergegraph_golden.npz to <in.bin> and compares <out.bin> with the golden values:
//   mergegraph_shim_test <in.bin> <out.bin>
// in:  int n, e; per node {int fixed; double R[9], t[3]}; per edge {int id1, id2, scaleId; double R[9], t[3]}
// out: per node {double newR[9], newt[3]}; per edge {double s}; then int threw (relaxPoseGraphs on the same graph: must be 1)
#include <cstdio>
#include <cstring>
#include <vector>

#include "slam/coslam_posegraph.h"

struct Node {
    bool fixed;
    double R[9], t[3], newR[9], newt[3];
};
struct Edge {
    int id1, id2;
    bool constraint, uncertainScale;
    double R[9], t[3], s;
    int scaleId;
};
struct Graph {
    int nNodes, nEdges;
    Node* poseNodes;
    Edge* poseEdges;
};

int main(int argc, char** argv) {
    if (argc < 3) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    int hdr[2];
    if (fread(hdr, sizeof(int), 2, f) != 2) return 2;
    std::vector<Node> nodes(hdr[0]);
    std::vector<Edge> edges(hdr[1]);
    for (int i = 0; i < hdr[0]; ++i) {
        int fx;
        if (fread(&fx, sizeof(int), 1, f) != 1 || fread(nodes[i].R, sizeof(double), 9, f) != 9 || fread(nodes[i].t, sizeof(double), 3, f) != 3) return 2;
        nodes[i].fixed = fx != 0;
        memset(nodes[i].newR, 0, sizeof(nodes[i].newR));
        memset(nodes[i].newt, 0, sizeof(nodes[i].newt));
    }
    for (int k = 0; k < hdr[1]; ++k) {
        int v[3];
        if (fread(v, sizeof(int), 3, f) != 3 || fread(edges[k].R, sizeof(double), 9, f) != 9 || fread(edges[k].t, sizeof(double), 3, f) != 3) return 2;
        edges[k].id1 = v[0], edges[k].id2 = v[1], edges[k].scaleId = v[2];
        edges[k].uncertainScale = edges[k].constraint = v[2] >= 0;
        edges[k].s = 0;
    }
    fclose(f);
    Graph g = {hdr[0], hdr[1], nodes.data(), edges.data()};
    try {
        relaxScaledPoseGraph(g);
    } catch (const std::exception& e) {
        fprintf(stderr, "%s\n", e.what());
        return 1;
    }
    int threw = 0;
    try {
        Graph g2 = g;
        std::vector<Node> copy(nodes);
        g2.poseNodes = copy.data();
        relaxPoseGraphs(&g2, 1);
    } catch (const std::exception&) {
        threw = 1;
    }
    f = fopen(argv[2], "wb");
    if (!f) return 2;
    for (int i = 0; i < g.nNodes; ++i) fwrite(nodes[i].newR, sizeof(double), 9, f), fwrite(nodes[i].newt, sizeof(double), 3, f);
    for (int k = 0; k < g.nEdges; ++k) fwrite(&edges[k].s, sizeof(double), 1, f);
    fwrite(&threw, sizeof(int), 1, f);
    fclose(f);
    printf("mergegraph shim ok (relaxPoseGraphs threw: %d)\n", threw);
    return 0;
}
