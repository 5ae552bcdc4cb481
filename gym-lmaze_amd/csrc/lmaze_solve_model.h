// The model of one grid maze as the kernels that plan it, score it and evaluate policies on it keep it (lmaze_solve.hip,
// lmaze_score.hip, lmaze_evaluate.hip): sixteen bits per cell, taken from transition_rule<VARIANT> itself, and what the kernels
// share of a problem's life in LDS -- the sync between two phases, where the rule's StepArgs and the vote words stand behind
// the two buffers, and the one-step backup of the two that sweep values.  The model is stated once, here, by asking the rule.
// The kernels' common opening is lmaze_problem_frame.h, included into each; their one launcher is at the end of this file.
#ifndef LMAZE_SOLVE_MODEL_H_
#define LMAZE_SOLVE_MODEL_H_

#include <math.h>

#include "lmaze_common.h"

namespace lmaze {

// a pair's four bits: which reward constant, the rule's done flag, whether the ball moved onto the target cell
enum { SOLVE_WALL = 0, SOLVE_MOVE = 1, SOLVE_GOAL = 2, SOLVE_EXCLUDED = 3, SOLVE_TERMINAL = 4, SOLVE_MOVED = 8 };
#define SOLVE_ALL_EXCLUDED 0x3333u
#define SOLVE_WALL_STATE 0x10000u     // the cell itself is 'W': q = v = 0, policy 0
#define SOLVE_VOTE_BYTES 64           // workgroup form: 2 x 4 vote words, 4 words of the last reduction
#define SOLVE_MODEL_BYTES ((sizeof(StepArgs) + 15) & ~(size_t)15)   // the StepArgs the rule is asked with, behind the two buffers

// The sixteen bits of cell s (a non-wall cell of a bordered layout has every target on the grid; the clamp keeps any other
// input inside the problem's own LDS: a clamped target is the cell itself)
template <int VARIANT>
__device__ __forceinline__ uint32_t solve_descriptor(const StepArgs& m, const uint8_t* lay, int G, int s, int gx, int gy) {
    if (lay[s] == 'W') return SOLVE_WALL_STATE;
    const int x = s / G, y = s - x * G;
    uint32_t d = 0;
#pragma unroll
    for (int act = 0; act < 4; ++act) {
        int ox, oy;
        decode_action(act, ox, oy);
        const int tx = clampi(x + ox, 0, G - 1), ty = clampi(y + oy, 0, G - 1);
        const uint8_t c = lay[tx * G + ty];
        int bx = x, by = y, bx1 = x, by1 = y;
        float r, r1;
        bool dn, dn1;
        transition_rule<VARIANT>(m, c, ox, oy, tx, ty, 0, 0.0f, gx, gy, bx, by, r, dn);
        transition_rule<VARIANT>(m, c, ox, oy, tx, ty, 0, 1.0f, gx, gy, bx1, by1, r1, dn1);
        uint32_t nib = SOLVE_EXCLUDED;
        if (__float_as_uint(r) == __float_as_uint(r1)) {
            const uint32_t rb = __float_as_uint(r);
            nib = rb == __float_as_uint(m.reward_goal) ? SOLVE_GOAL : (rb == __float_as_uint(m.reward_move) ? SOLVE_MOVE : SOLVE_WALL);
            nib |= (dn ? SOLVE_TERMINAL : 0) | (bx * G + by != s ? SOLVE_MOVED : 0);
        }
        d |= nib << (4 * act);
    }
    return d;
}

// r + gamma * v with the product and the sum rounded separately, as returns_step (lmaze_aux.hip): never an fma
__device__ __forceinline__ float solve_backup(float r, float gamma, float v) {
#pragma clang fp contract(off)
    const float discounted = gamma * v;
    return r + discounted;
}

// Q_k(s, .) from V_(k-1) for a non-wall cell: r on a terminal pair, else r + gamma * V_(k-1)(next), -inf on an excluded pair.
// Args: SolveArgs or EvaluateArgs (grid, gamma and the three rewards).
template <class Args>
__device__ __forceinline__ void solve_action_values(const Args& a, uint32_t d, int s, const float* vo, float (&q)[4]) {
    const int G = a.grid;
#pragma unroll
    for (int act = 0; act < 4; ++act) {
        const uint32_t nib = (d >> (4 * act)) & 15u, sel = nib & 3u;
        const int step = act == 0 ? -G : (act == 1 ? G : (act == 2 ? -1 : 1));
        const float r = sel == SOLVE_GOAL ? a.reward_goal : (sel == SOLVE_MOVE ? a.reward_move : a.reward_wall);
        const float vn = vo[(nib & SOLVE_MOVED) ? s + step : s];
        const float backed = (nib & SOLVE_TERMINAL) ? r : solve_backup(r, a.gamma, vn);
        q[act] = sel == SOLVE_EXCLUDED ? -INFINITY : backed;
    }
}

// what one problem's threads wait on between two phases that exchange data through its LDS
template <bool WAVE>
__device__ __forceinline__ void solve_sync() {
    if constexpr (WAVE) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    } else {
        __syncthreads();
    }
}

// One launch site for the four families (solve, score, evaluate, occupancy).  Family: its Args type and
// kernel<VARIANT, CPL, WAVE>(), the instantiation's address.
template <class Family, int VARIANT, int CPL, bool WAVE>
static hipError_t problem_launch(const typename Family::Args& a, const SolvePlan& p, hipStream_t s) {
    hipLaunchKernelGGL((Family::template kernel<VARIANT, CPL, WAVE>()), dim3((unsigned)p.grid), dim3(LMAZE_BLOCK), (size_t)p.lds_bytes, s, a);
    return hipGetLastError();
}

template <class Family, int VARIANT>
static hipError_t problem_dispatch(const typename Family::Args& a, const SolvePlan& p, hipStream_t s) {
    if (p.wave) {
        switch (p.cells_per_lane) {
            case 1: return problem_launch<Family, VARIANT, 1, true>(a, p, s);
            case 2: return problem_launch<Family, VARIANT, 2, true>(a, p, s);
            default: return problem_launch<Family, VARIANT, 4, true>(a, p, s);
        }
    }
    switch (p.cells_per_lane) {
        case 2: return problem_launch<Family, VARIANT, 2, false>(a, p, s);
        case 4: return problem_launch<Family, VARIANT, 4, false>(a, p, s);
        case 8: return problem_launch<Family, VARIANT, 8, false>(a, p, s);
        default: return problem_launch<Family, VARIANT, 16, false>(a, p, s);
    }
}

// the plan is plan_solve's for every family: the same two buffers of S words per problem, the same model and vote words
template <class Family>
static hipError_t launch_problems(int variant, const typename Family::Args& a, hipStream_t s) {
    if (a.problems == 0) return hipSuccess;
    const SolvePlan p = plan_solve(a.grid, a.problems);
    if (!grid_ok(p.grid)) return hipErrorInvalidConfiguration;
    return variant == LMAZE_VARIANT_V3 ? problem_dispatch<Family, LMAZE_VARIANT_V3>(a, p, s)
                                       : problem_dispatch<Family, LMAZE_VARIANT_V0>(a, p, s);
}

}  // namespace lmaze
#endif
