// history_view.h -- what the result export (export.hip) reads of a cs_track_history (poseupdate.hip owns the handle): the store's
// ring, the whole-run archive behind it and the linked-segment pools.  Internal to the library.
#pragma once

#include "cs_common.h"

struct CsHistView {
    int device, nCams, N, H, head, stored, lastFrame, firstFrame;
    const double *xy, *R, *t;        // ring [nCams][H][2N] / [9] / [3]
    int archCap, archCount, archFirst;
    const double *archXY, *archR, *archT;   // archive [nCams][archCap][2N] / [9] / [3]
    const int4* segPool;   // [nCams][segCap]
    const int* segCount;   // [nCams] (device)
    int segCap;
};
void cs_history_view(const cs_track_history* h, CsHistView* v);
