// The selection rule of the closed-loop two-level rollout of v5/v6 (lmaze_v5_rollout_policy: include/lmaze.h), shared by the
// kernel (lmaze_foveal_body.h, its LMAZE_FOVEAL_HIER_SITE) and by a host-compiled program (tests/csrc/hier_select_host.cpp,
// CPU suite) that runs the same text against a numpy restatement: the two keys and the two selections.
#ifndef LMAZE_HIER_SELECT_H_
#define LMAZE_HIER_SELECT_H_

#include "lmaze_foveal_select.h"

#define LMAZE_HIER_OFFSETS 100   // keys of the "offset" controller: 10 x 10 foveal-goal offsets
#define LMAZE_HIER_GOALS 25      // planner goals: the cells of the 5 x 5 window
#define LMAZE_HIER_ACTIONS 4     // controller actions

// The planner's key: the rule of state_keys() -- layout row and ball, each clamped into the table.
LMAZE_HD int lmaze_hier_planner_key(int lid, int bx, int by, int G, int L) { return lmaze_foveal_key(lid, bx, by, G, L); }

// One axis of the foveal goal's offset from the ball, clamp(fg - b + 4, 0, 9).  An undisturbed env has fg - b in -4..5; the
// difference is taken in 64 bits so that any pair of int32 coordinates (a loaded state) is defined.
LMAZE_HD int lmaze_hier_axis(int fg, int b) {
    const int64_t o = (int64_t)fg - (int64_t)b + 4;
    return o < 0 ? 0 : (o > 9 ? 9 : (int)o);
}

// d = ox * 10 + oy, 0..99.
LMAZE_HD int lmaze_hier_offset(int fgx, int fgy, int bx, int by) { return lmaze_hier_axis(fgx, bx) * 10 + lmaze_hier_axis(fgy, by); }

// The controller's key.  controller_key 0 ("offset"): d, 100 keys; 1 ("cell"): kp * 100 + d with kp the planner key of the
// current state -- the controller's full Markov state, 100 L G^2 keys.
LMAZE_HD int lmaze_hier_controller_key(int controller_key, int kp, int d) { return controller_key ? kp * LMAZE_HIER_OFFSETS + d : d; }

// The planner's goal: the table's id, or -- where rz < planner_epsilon -- floor(rw * 25 / 2^32).  planner_epsilon == 0 ignores
// the draw.  The id is passed through: above 24 the plannerStep is skipped.
LMAZE_HD int lmaze_hier_goal(int greedy, uint32_t rz, uint32_t rw, uint32_t planner_epsilon) {
    return lmaze_foveal_choose(greedy, rz, rw, planner_epsilon, LMAZE_HIER_GOALS);
}

// The controller's action: the table's id, or -- where rx < epsilon -- ry >> 30.  epsilon == 0 ignores the draw.  The id is
// passed through: above 3 the step does not move.
LMAZE_HD int lmaze_hier_action(int greedy, uint32_t rx, uint32_t ry, uint32_t epsilon) {
    return lmaze_foveal_choose(greedy, rx, ry, epsilon, LMAZE_HIER_ACTIONS);
}

#endif  // LMAZE_HIER_SELECT_H_
