// ref_mergematch_offpath.h -- what src/app/SL_MergeCameraGroup.cpp names of un-vendored LibVisualSLAM beyond oracle/ref_shim/, for
// tests/cxx/ref_mergematch_test.cpp (force-included on its compile line; ref_merge_offpath.h is the constraints driver's).  Here the
// front of matchMergableCameras is ON the path: SURF detection / matching and the essential matrix are plain functions that the driver
// defines as stand-ins replaying a scene's recorded inputs, getMatchedPts gets its body there, and the call of genMergeInfoVer2 at :416 is
// redirected (on the compile line) to a recorder of its five arguments.  The first block stays off the path: declared, never defined.
#pragma once
#include <algorithm>
#include <functional>
#include <vector>

#include "geometry/SL_BundleAdjust.h"
#include "imgproc/SL_Image.h"
#include "matching/SL_Matching.h"
#include "math/SL_Matrix.h"

void bundleAdjustRobust(int nCamsCon, std::vector<Mat_d>& Ks, std::vector<Mat_d>& Rs, std::vector<Mat_d>& Ts, int nPtsCon,
                        std::vector<Point3d>& pts, std::vector<std::vector<Meas2D> >& meas, double maxErr, int maxIter, int innerMaxIter);

template <class... A> void poly2Mask(A&&...);
template <class... A> void decompEMat(A&&...);
template <class... A> void getCameraCenterAxes(A&&...);
template <class... A> double innerProd3(A&&...);
template <class... A> void findConnectedComponents(A&&...);
template <class... A> void printMat(A&&...);
void sortWithInd(int n, int* vals, int* ind, bool ascending);
void matEyes(int n, Mat_d& I);
void matZeros(int m, int n, Mat_d& Z);

// on the path of matchMergableCameras: stand-ins (replay) and our definitions, bodies in the driver
int detectSURFPoints(const ImgG& img, Mat_d& surfPts, std::vector<float>& surfDesc);
int matchSurf(int dimDesc, std::vector<float>& desc1, std::vector<float>& desc2, Matching& matches, double ratio, double maxDist);
int estimateEMat(const double* K1, const double* K2, const Mat_d& pts1, const Mat_d& pts2, const Matching& matches, double* E, int nRansac,
                 double maxEpiErr, int minInlierNum);
int evaluateEMat(int n, const double* pts2, const double* pts1, const double* F, double maxEpiErr, double& epiErr, unsigned char* inlierFlag);
void getMatchedPts(const Matching& matches, const Mat_d& pts1, const Mat_d& pts2, Mat_d& m1, Mat_d& m2);
bool refRecordGenMergeInfo(int gId1, int gId2, int iCam, int jCam, const Matching& featMatches);
