// The sampling rule of the closed-loop two-level rollout of v5/v6 (lmaze_v5_rollout_sample: include/lmaze.h), shared by the
// kernel (lmaze_foveal_body.h, its LMAZE_FOVEAL_HIER_SAMPLE_SITE, through hier_smp_goal / hier_smp_act of lmaze_foveal_defs.h)
// and by a host-compiled program (tests/csrc/hier_sample_host.cpp, CPU suite) that runs the same text against a numpy
// restatement: the two row formats and the two compare-sums.  The keys are lmaze_hier_select.h's, the sum lmaze_foveal_sample.h's.
#ifndef LMAZE_HIER_SAMPLE_H_
#define LMAZE_HIER_SAMPLE_H_

#include "lmaze_foveal_sample.h"
#include "lmaze_hier_select.h"

#define LMAZE_HIER_SAMPLE_CROW 4    // words of a controller row: c0, c1, c2 and a reserved word (the grid envs' and v1's format)
#define LMAZE_HIER_SAMPLE_PROW 24   // words of a planner row: c0 .. c23 (the v2/v4 format)

// Keys of the controller table: 100 ("offset") or 100 L G^2 ("cell").
LMAZE_HD int lmaze_hier_sample_controller_keys(int controller_key, int L, int G) {
    return controller_key ? LMAZE_HIER_OFFSETS * L * G * G : LMAZE_HIER_OFFSETS;
}

// The planner's goal: how many of the row's 24 thresholds the draw word r.z has reached, 0..24 -- never out of range, so no
// plannerStep is ever skipped.
LMAZE_HD int lmaze_hier_sample_goal(const uint32_t* row, uint32_t rz) {
    return lmaze_foveal_sample_action(row, LMAZE_HIER_GOALS - 1, rz);
}

// The controller's action: how many of the row's first 3 thresholds the draw word r.x has reached, 0..3; the reserved word is
// not compared.
LMAZE_HD int lmaze_hier_sample_action(const uint32_t* row, uint32_t rx) {
    return lmaze_foveal_sample_action(row, LMAZE_HIER_ACTIONS - 1, rx);
}

#endif  // LMAZE_HIER_SAMPLE_H_
