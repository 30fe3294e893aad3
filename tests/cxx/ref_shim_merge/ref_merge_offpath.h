// ref_merge_offpath.h -- what src/app/SL_MergeCameraGroup.cpp names of un-vendored LibVisualSLAM beyond oracle/ref_shim/, for
// tests/cxx/ref_mergeconstraints_test.cpp (force-included on its compile line).  Everything in the first block is OFF the path of
// genMergeInfoVer2 (SURF, the essential matrix, the overlap mask, the group components, printing): declared so the file compiles, never
// defined -- --gc-sections drops the functions that call them.  The second block is on the path and gets bodies in the driver.
#pragma once
#include <algorithm>
#include <functional>
#include <vector>

#include "geometry/SL_BundleAdjust.h"
#include "math/SL_Matrix.h"

// The solver stand-in (bundleAdjustRobust has no source in the reference tree): a plain function with the call's exact types, which
// overload resolution prefers at :646-647 to the product's template of include/shim/geometry/SL_BundleAdjust.h.  The driver defines it:
// it records the first call's arguments and changes nothing.
void bundleAdjustRobust(int nCamsCon, std::vector<Mat_d>& Ks, std::vector<Mat_d>& Rs, std::vector<Mat_d>& Ts, int nPtsCon,
                        std::vector<Point3d>& pts, std::vector<std::vector<Meas2D> >& meas, double maxErr, int maxIter, int innerMaxIter);

template <class... A> void poly2Mask(A&&...);
template <class... A> int estimateEMat(A&&...);
template <class... A> int evaluateEMat(A&&...);
template <class... A> void decompEMat(A&&...);
template <class... A> void getCameraCenterAxes(A&&...);
template <class... A> double innerProd3(A&&...);
template <class... A> void getMatchedPts(A&&...);
template <class... A> int detectSURFPoints(A&&...);
template <class... A> int matchSurf(A&&...);
template <class... A> void findConnectedComponents(A&&...);
template <class... A> void printMat(A&&...);

// on the path: getUnMergedFeatureTracks (:860), getRigidTransFromToWithEMat (:1215-1216)
void sortWithInd(int n, int* vals, int* ind, bool ascending);
void matEyes(int n, Mat_d& I);
void matZeros(int m, int n, Mat_d& Z);
