// Kernel arguments and launchers of the MLP classifier's step (classifier.hip; the C entry point in classifier_unit.cpp;
// include/ocrl_hip_classifier.h is the specification).  The head is the Q head of dqn.h with A = the number of classes: the same
// AcnetArgs on the tile code of acnet_tile.h, the same host side (acnet_host.h) and the same workspace.
#pragma once
#include "../../include/ocrl_hip_classifier.h"
#include "dqn.h"

// the cross-entropy's inputs; backward == 0 evaluates (the tiles stop after the loss)
struct ClfCeArgs {
    const long long* labels;                          // [B]
    int backward;
};

int clf_ce_launch(const AcnetArgs& a, const ClfCeArgs& s, hipStream_t st);
