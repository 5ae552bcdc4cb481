// The action law of a state as the two linear kernels read it (lmaze_evaluate.hip, lmaze_occupancy.hip): the one statement of
// include/lmaze.h's weight rule, from the table a closed-loop rollout would run to the four probabilities of a cell.
#ifndef LMAZE_POLICY_PROBS_H_
#define LMAZE_POLICY_PROBS_H_

#include "lmaze_common.h"
#include "lmaze_learn.h"
#include "lmaze_solve_model.h"

namespace lmaze {

// The four probabilities of a cell.  w_a in units of 2^-34: the epsilon-greedy mixture of lmaze_rollout_policy or the differences
// of lmaze_rollout_sample's three thresholds taken in ascending order; w'_a = 0 on an excluded pair; p_a = fl(fl(w'_a) / fl(W)),
// W the integer sum.  A wall state has no probabilities, and W == 0 leaves none either.
// Args: EvaluateArgs or OccupancyArgs (thresholds, q, policy, epsilon).
template <class Args>
__device__ __forceinline__ void evaluate_probs(const Args& a, int64_t row, uint32_t d, float (&p)[4]) {
    uint64_t w[4];
    if (a.thresholds) {
        const uint4 c = a.thresholds[row];                        // one 128-bit load per state; word 3 is not looked at
        // The sampler counts the words that r reaches, (r >= c0) + (r >= c1) + (r >= c2), so the action law of a row is that
        // of its three words in ascending order, whatever order they are stored in: a sort of three, once per state.
        const uint32_t lo = min(c.x, c.y), hi = max(c.x, c.y);
        const uint32_t s0 = min(lo, c.z), s2 = max(hi, c.z), s1 = max(lo, min(hi, c.z));
        w[0] = 4ull * s0;
        w[1] = 4ull * (s1 - s0);
        w[2] = 4ull * (s2 - s1);
        w[3] = 4ull * (0x100000000ull - s2);
    } else {
        uint32_t greedy;
        if (a.q) {
            const float4 r4 = a.q[row];
            const float r[4] = {r4.x, r4.y, r4.z, r4.w};
            int first;
            lmaze_q_first_max(r, &first);
            greedy = (uint32_t)first;
        } else {
            greedy = a.policy[row];                               // above 3: the greedy share goes to no action
        }
        const uint64_t e = a.epsilon;
#pragma unroll
        for (int act = 0; act < 4; ++act) w[act] = e + (greedy == (uint32_t)act ? 4ull * (0x100000000ull - e) : 0ull);
    }
    uint64_t W = 0;
#pragma unroll
    for (int act = 0; act < 4; ++act) {
        if ((d & SOLVE_WALL_STATE) || ((d >> (4 * act)) & 3u) == SOLVE_EXCLUDED) w[act] = 0;
        W += w[act];
    }
    const float fW = __ull2float_rn(W);
#pragma unroll
    for (int act = 0; act < 4; ++act) p[act] = w[act] ? __fdiv_rn(__ull2float_rn(w[act]), fW) : 0.0f;
}

}  // namespace lmaze
#endif
