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
    extern __shared__ __align__(16) unsigned char solve_lds[];
#define PROBLEM_LDS solve_lds
#define PROBLEM_WORD float
#define PROBLEM_AT_COPY(s) buf[s] = a.v_init ? a.v_init[base + s] : 0.0f   // V_0 goes into the first buffer
#define PROBLEM_AT_DESC(j, s, d)
#include "lmaze_problem_frame.h"
    float* const vbuf = buf;

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

// what lmaze_describe_solve, _score and _evaluate print: the kernel's name and the plan
int describe_problems_plan(const char* kernel, int variant, const SolvePlan& p, char* text, int32_t len) {
    if (!text || len < 1) return LMAZE_E_NULL;
    snprintf(text, (size_t)len, "%s<%s, %s, %d> grid=%lld block=%d lds=%lld problems_per_workgroup=%d", kernel,
             variant == LMAZE_VARIANT_V3 ? "v3" : "v0", p.wave ? "wave" : "workgroup", p.cells_per_lane, (long long)p.grid, LMAZE_BLOCK,
             (long long)p.lds_bytes, p.problems_per_workgroup);
    return 0;
}

struct SolveFamily {
    using Args = SolveArgs;
    template <int VARIANT, int CPL, bool WAVE>
    static constexpr auto kernel() { return &solve_kernel<VARIANT, CPL, WAVE>; }
};
hipError_t launch_solve(int variant, const SolveArgs& a, hipStream_t s) { return launch_problems<SolveFamily>(variant, a, s); }

}  // namespace lmaze
