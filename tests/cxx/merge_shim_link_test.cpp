// Compiles include/shim/app/CoSLAMMergeCheck.h (MergeCameraGroup::checkPossibleMergable's shape over the C-ABI) against libcoslam_hip.so
// and checks, with or without a GPU, that a call the library must refuse fails loudly with the C-ABI's error text and leaves the list empty.
#include <cstdio>
#include <cstring>
#include <stdexcept>

#include "app/CoSLAMMergeCheck.h"

int main() {
    static_assert(sizeof(cs_merge_info) == 24, "MergeInfo");
    static_assert(sizeof(cs_merge_candidates) == 16 + 256 * 24 + 64 + 1024 + 1024 + 256 + 2048, "cs_merge_candidates");
    CoSLAMMergeCheck merger(2, 100, 1000);
    merger.setImageSize(0, 640, 480);
    merger.setImageSize(1, 640, 480);
    merger.setCurrentFrame(5, 0);   // no record of the groups, no tables: refused before anything touches a device
    bool threw = false;
    try {
        merger.checkPossibleMergable(10, 0.5, 6.0);
    } catch (const std::runtime_error& e) {
        threw = strstr(e.what(), "null") != 0 || strstr(e.what(), "failed") != 0 || strstr(e.what(), "device") != 0;
        printf("refused: %s\n", e.what());
    }
    if (!threw || merger.m_nMergeInfo != 0) return 1;
    try {
        merger.setImageSize(2, 640, 480);
        return 1;
    } catch (const std::runtime_error&) {
    }
    printf("merge shim ok (%zu-byte record)\n", sizeof(cs_merge_candidates));
    return 0;
}
