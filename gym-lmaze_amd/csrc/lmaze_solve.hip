// lmaze_solve.hip -- value iteration over the grid mazes (lmaze_solve / lmaze_describe_solve, include/lmaze.h).
//
// One problem = one maze of S = G*G states and four actions, deterministic.  The model is not restated here: every
// (cell, action) pair is pushed once through transition_rule<VARIANT> (lmaze_common.h: v0:172-195, v0:246-249, v3:224-265,
// v3:398) with a step count that trips no limit, and what comes back -- where the ball is, which of the three reward
// constants it was paid, the rule's own done flag -- is packed into four bits per pair, sixteen per cell, kept in registers
// by the lane that owns the cell.  A pair whose reward depends on the reward that came in (v0's sticky pair: the rule is run
// with two different incoming rewards and answers differently) has no reward of its own and is excluded.
//
// A problem then lives in LDS for the whole solve: two V buffers, Jacobi sweeps between them, four neighbour reads and one
// write per cell and sweep.  Global memory is read at the start (layout, goal, v_init) and written at the end.  Two forms,
// picked from G alone (plan_solve):
//   wave        G*G <= 256: a wave per problem, four problems per workgroup, 1-4 cells per lane.  The lanes of a wave run in
//               lockstep and the LDS serves one wave's operations in order, so a sweep needs a compiler fence and no
//               workgroup barrier, and a wave whose problem has settled leaves on its own.
//   workgroup   above: a workgroup per problem, 2-16 cells per lane, one __syncthreads() per sweep.  The "unchanged" vote is
//               a word per wave in LDS, written before that barrier and read by every thread after it, so all 256 threads
//               take the same exit; the two parities of the words keep a fast wave's next vote off a slow wave's read.
#include <limits.h>
#include <math.h>
#include <stdio.h>

#include "lmaze_common.h"
#include "lmaze_solve_model.h"   // the sixteen bits of a cell, solve_sync, where the model and the votes stand in LDS

namespace lmaze {

// Q_k(s, .) from V_(k-1) (solve_action_values, lmaze_solve_model.h), the first maximum by strict '>' and its action
__device__ __forceinline__ float solve_cell(const SolveArgs& a, uint32_t d, int s, const float* vo, float (&q)[4], int& pol) {
    solve_action_values(a, d, s, vo, q);
    float best = q[0];
    pol = 0;
#pragma unroll
    for (int act = 1; act < 4; ++act)
        if (q[act] > best) { best = q[act]; pol = act; }
    if ((d & SOLVE_ALL_EXCLUDED) == SOLVE_ALL_EXCLUDED) { best = 0.0f; pol = 0; }
    if (d & SOLVE_WALL_STATE) {
        q[0] = q[1] = q[2] = q[3] = 0.0f;
        best = 0.0f;
        pol = 0;
    }
    return best;
}

template <int VARIANT, int CPL, bool WAVE>
__global__ __launch_bounds__(LMAZE_BLOCK) void solve_kernel(const SolveArgs a) {
    constexpr int TPP = WAVE ? 64 : LMAZE_BLOCK;        // threads per problem
    constexpr int PPW = LMAZE_BLOCK / TPP;              // problems per workgroup
    constexpr int SP = CPL * TPP;                       // floats of one V buffer, >= S
    extern __shared__ __align__(16) unsigned char solve_lds[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int t = WAVE ? lane : (int)threadIdx.x;
    const int64_t p = (int64_t)blockIdx.x * PPW + (WAVE ? wave : 0);
    // wave form: a whole wave without a problem, and no barrier in that form waits for it; workgroup form: never
    if (p >= a.problems) return;
    float* const vbuf = reinterpret_cast<float*>(solve_lds) + (WAVE ? wave : 0) * 2 * SP;
    uint32_t* const vote = reinterpret_cast<uint32_t*>(solve_lds + (size_t)PPW * 2 * SP * sizeof(float) + SOLVE_MODEL_BYTES);   // workgroup form only
    const int G = a.grid, S = G * G;
    const int64_t base = p * S;

    // the layout's bytes borrow the second V buffer until the descriptors are built; V_0 goes into the first
    uint8_t* const lay = reinterpret_cast<uint8_t*>(vbuf + SP);
    const uint8_t* const lay_g = a.layouts + (a.per_env ? base : 0);
#pragma unroll
    for (int j = 0; j < CPL; ++j) {
        const int s = t + j * TPP;
        if (s < S) {
            lay[s] = lay_g[s];
            vbuf[s] = a.v_init ? a.v_init[base + s] : 0.0f;
        }
    }
    int gx = -1, gy = -1;
    if (VARIANT == LMAZE_VARIANT_V3) {
        const int2 g = a.goal[p];
        gx = g.x;
        gy = g.y;
    }
    // What transition_rule reads when it is asked for the model: the three rewards, and a step_limit that the step count it is
    // asked with (0) never meets -- INT_MAX: neither v0's "==" nor v3's ">"; the limit is not in the model.  The struct stands
    // in LDS: v3's rule selects between two of its rewards by address, which would pin a private copy in scratch.  Every wave
    // writes the same four words and reads them behind its own fence.
    StepArgs* const m = reinterpret_cast<StepArgs*>(solve_lds + (size_t)PPW * 2 * SP * sizeof(float));
    if (lane == 0) {
        m->reward_wall = a.reward_wall;
        m->reward_move = a.reward_move;
        m->reward_goal = a.reward_goal;
        m->step_limit = INT_MAX;
    }
    solve_sync<WAVE>();
    uint32_t desc[CPL];
#pragma unroll
    for (int j = 0; j < CPL; ++j) {
        const int s = t + j * TPP;
        desc[j] = s < S ? solve_descriptor<VARIANT>(*m, lay, G, s, gx, gy) : SOLVE_WALL_STATE;
    }
    solve_sync<WAVE>();

    int cur = 0, k = 0;                // V_(k-1) is vbuf[cur]
    uint32_t dbits;
    for (;;) {
        ++k;
        const float* const vo = vbuf + cur * SP;
        float* const vn = vbuf + (cur ^ 1) * SP;
        bool changed = false;
        dbits = 0;
#pragma unroll
        for (int j = 0; j < CPL; ++j) {
            const int s = t + j * TPP;
            if (s < S) {
                float q[4];
                int pol;
                const float best = solve_cell(a, desc[j], s, vo, q, pol);
                const float old = vo[s];
                vn[s] = best;
                changed |= __float_as_uint(best) != __float_as_uint(old);
                // |V_k - V_(k-1)| as bits: non-negative floats order as unsigned integers
                dbits = max(dbits, __float_as_uint(best - old) & 0x7FFFFFFFu);
            }
        }
        bool any = __ballot(changed) != 0ull;
        if constexpr (WAVE) {
            solve_sync<true>();
        } else {
            uint32_t* const mine = vote + (k & 1) * 4;
            if (lane == 0) mine[wave] = any ? 1u : 0u;
            __syncthreads();           // V_k and the four votes; every thread of the workgroup is here, every sweep
            any = (mine[0] | mine[1] | mine[2] | mine[3]) != 0u;
        }
        cur ^= 1;
        if (!any || k == a.sweeps) break;   // the same answer in every thread of the problem
    }

    // Q_k of the last sweep from V_(k-1), which the other buffer still holds
    const float* const vo = vbuf + (cur ^ 1) * SP;
#pragma unroll
    for (int j = 0; j < CPL; ++j) {
        const int s = t + j * TPP;
        if (s < S) {
            float q[4];
            int pol;
            const float best = solve_cell(a, desc[j], s, vo, q, pol);
            if (a.q) a.q[base + s] = make_float4(q[0], q[1], q[2], q[3]);
            if (a.v) a.v[base + s] = best;
            if (a.policy) a.policy[base + s] = (uint8_t)pol;
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) dbits = max(dbits, (uint32_t)__shfl_xor((int)dbits, off, 64));
    if constexpr (!WAVE) {
        uint32_t* const red = vote + 8;
        if (lane == 0) red[wave] = dbits;
        __syncthreads();
        dbits = max(max(red[0], red[1]), max(red[2], red[3]));
    }
    if (t == 0) {
        if (a.sweeps_run) a.sweeps_run[p] = k;
        if (a.delta) a.delta[p] = __uint_as_float(dbits);
    }
}

SolvePlan plan_solve(int32_t G, int64_t problems) {
    const int S = G * G;
    SolvePlan p;
    p.wave = S <= 256;
    if (p.wave) p.cells_per_lane = S <= 64 ? 1 : (S <= 128 ? 2 : 4);
    else p.cells_per_lane = S <= 512 ? 2 : (S <= 1024 ? 4 : (S <= 2048 ? 8 : 16));
    p.problems_per_workgroup = p.wave ? LMAZE_BLOCK / 64 : 1;
    p.grid = (problems + p.problems_per_workgroup - 1) / p.problems_per_workgroup;
    const int64_t threads = p.wave ? 64 : LMAZE_BLOCK;
    p.lds_bytes = (int64_t)p.problems_per_workgroup * 2 * p.cells_per_lane * threads * (int64_t)sizeof(float) + (int64_t)SOLVE_MODEL_BYTES +
                  (p.wave ? 0 : SOLVE_VOTE_BYTES);
    return p;
}

int describe_solve(int variant, const SolvePlan& p, char* text, int32_t len) {
    if (!text || len < 1) return LMAZE_E_NULL;
    snprintf(text, (size_t)len, "solve_kernel<%s, %s, %d> grid=%lld block=%d lds=%lld problems_per_workgroup=%d",
             variant == LMAZE_VARIANT_V3 ? "v3" : "v0", p.wave ? "wave" : "workgroup", p.cells_per_lane, (long long)p.grid, LMAZE_BLOCK,
             (long long)p.lds_bytes, p.problems_per_workgroup);
    return 0;
}

template <int VARIANT, int CPL, bool WAVE>
static hipError_t solve_launch(const SolveArgs& a, const SolvePlan& p, hipStream_t s) {
    hipLaunchKernelGGL((solve_kernel<VARIANT, CPL, WAVE>), dim3((unsigned)p.grid), dim3(LMAZE_BLOCK), (size_t)p.lds_bytes, s, a);
    return hipGetLastError();
}

template <int VARIANT>
static hipError_t solve_dispatch(const SolveArgs& a, const SolvePlan& p, hipStream_t s) {
    if (p.wave) {
        switch (p.cells_per_lane) {
            case 1: return solve_launch<VARIANT, 1, true>(a, p, s);
            case 2: return solve_launch<VARIANT, 2, true>(a, p, s);
            default: return solve_launch<VARIANT, 4, true>(a, p, s);
        }
    }
    switch (p.cells_per_lane) {
        case 2: return solve_launch<VARIANT, 2, false>(a, p, s);
        case 4: return solve_launch<VARIANT, 4, false>(a, p, s);
        case 8: return solve_launch<VARIANT, 8, false>(a, p, s);
        default: return solve_launch<VARIANT, 16, false>(a, p, s);
    }
}

hipError_t launch_solve(int variant, const SolveArgs& a, hipStream_t s) {
    if (a.problems == 0) return hipSuccess;
    const SolvePlan p = plan_solve(a.grid, a.problems);
    if (!grid_ok(p.grid)) return hipErrorInvalidConfiguration;
    return variant == LMAZE_VARIANT_V3 ? solve_dispatch<LMAZE_VARIANT_V3>(a, p, s) : solve_dispatch<LMAZE_VARIANT_V0>(a, p, s);
}

}  // namespace lmaze
