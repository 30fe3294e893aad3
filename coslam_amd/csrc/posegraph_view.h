// posegraph_view.h -- what a device-side guard reads of a cs_posegraph (posegraph.hip owns the handle): the per-component status words
// the last relaxation launch wrote (0 = solved; cs_posegraph_status reads the same words on the host).  Internal to the library.
#pragma once

#include "cs_common.h"

void cs_posegraph_status_words(const cs_posegraph* g, const int** d_status, int* n);
