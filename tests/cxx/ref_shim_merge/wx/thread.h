// Empty stand-in: the reference includes this header by name; nothing of it is on the path of genMergeInfoVer2
// (tests/cxx/ref_mergeconstraints_test.cpp).  The few helpers the file names are declared in ref_merge_offpath.h.
#pragma once
