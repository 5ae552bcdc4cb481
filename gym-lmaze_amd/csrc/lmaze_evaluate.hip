// lmaze_evaluate.hip -- exact policy evaluation on the grid mazes (lmaze_evaluate / lmaze_describe_evaluate, include/lmaze.h):
// V^pi and Q^pi of the stochastic table a closed-loop rollout would run, the linear twin of lmaze_solve.hip.
//
// One problem = one maze of S = G*G states and one table.  The model is solve_kernel's, from the function it uses
// (solve_descriptor over transition_rule, lmaze_solve_model.h): sixteen bits per cell in a register of the lane that owns the
// cell.  The table is read from global memory once, at setup, and reduced there to the four probabilities of the cell --
// integer weights in units of 2^-34, the weight on an excluded pair dropped, one correctly rounded division each -- which stay
// in registers beside the descriptor for the whole solve, in every form: 16 bytes per cell in LDS would add four reads per cell
// and sweep to the five the sweep already makes, and give the kernel an LDS size other than plan_solve's (not built, not timed).
//
// The rest is solve_kernel's: two V buffers in LDS, Jacobi sweeps between them, the layout's bytes borrowing the second while
// the descriptors are built, the plan of plan_solve (a wave per problem while S <= 256, a workgroup per problem above), one
// fence or one barrier per sweep, and an exit that every thread of a problem takes in the same sweep.  A vote carries two bits:
// "a value changed" and "a value moved by more than tol".
#include <limits.h>
#include <math.h>
#include <stdio.h>

#include "lmaze_common.h"
#include "lmaze_learn.h"
#include "lmaze_policy_probs.h"
#include "lmaze_solve_model.h"

namespace lmaze {

// Q_k(s, .) from V_(k-1) and V_k(s) = sum_a p_a Q_k(s, a): in the order a = 0..3, from the first term itself, over the actions
// that carry weight (an excluded pair carries none, so -inf * 0 never occurs); every product and sum rounded on its own
__device__ __forceinline__ float evaluate_cell(const EvaluateArgs& a, uint32_t d, const float (&p)[4], int s, const float* vo,
                                               float (&q)[4]) {
#pragma clang fp contract(off)
    if (d & SOLVE_WALL_STATE) {
        q[0] = q[1] = q[2] = q[3] = 0.0f;
        return 0.0f;
    }
    solve_action_values(a, d, s, vo, q);
    float v = 0.0f;
    bool first = true;
#pragma unroll
    for (int act = 0; act < 4; ++act) {
        if (p[act] != 0.0f) {
            const float term = p[act] * q[act];
            const float sum = v + term;
            v = first ? term : sum;
            first = false;
        }
    }
    return v;
}

// Sixteen cells per lane keep 80 registers for the whole solve and the compiler hoists what else a sweep repeats (targets,
// rewards); asked for two waves per SIMD it stays inside 256 registers without scratch, so two workgroups share a CU and one
// sweeps while the other stands at its barrier.
template <int VARIANT, int CPL, bool WAVE>
__global__ __launch_bounds__(LMAZE_BLOCK, (CPL == 16 ? 2 : 1)) void evaluate_kernel(const EvaluateArgs a) {
    extern __shared__ __align__(16) unsigned char evaluate_lds[];
    float prob[CPL][4];
#define PROBLEM_LDS evaluate_lds
#define PROBLEM_WORD float
#define PROBLEM_AT_COPY(s) buf[s] = a.v_init ? a.v_init[base + s] : 0.0f   // V_0 goes into the first buffer
#define PROBLEM_AT_CELL(j) prob[j][0] = prob[j][1] = prob[j][2] = prob[j][3] = 0.0f   // like a wall state: no probabilities
#define PROBLEM_AT_DESC(j, s, d) evaluate_probs(a, base + s, d, prob[j])
#include "lmaze_problem_frame.h"
    float* const vbuf = buf;

    // tol as a bit pattern: deltas are non-negative floats or NaNs, which order as unsigned integers with every NaN on top
    const bool use_tol = a.tol > 0.0f;
    const uint32_t tol_bits = __float_as_uint(a.tol);
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
                const float v = evaluate_cell(a, desc[j], prob[j], s, vo, q);
                const float old = vo[s];
                vn[s] = v;
                changed |= __float_as_uint(v) != __float_as_uint(old);
                dbits = max(dbits, __float_as_uint(v - old) & 0x7FFFFFFFu);
            }
        }
        const bool far = !use_tol || dbits > tol_bits;
        bool any_changed = __ballot(changed) != 0ull, any_far = __ballot(far) != 0ull;
        if constexpr (WAVE) {
            solve_sync<true>();
        } else {
            uint32_t* const mine = vote + (k & 1) * 4;
            if (lane == 0) mine[wave] = (any_changed ? 1u : 0u) | (any_far ? 2u : 0u);
            __syncthreads();           // V_k and the four votes; every thread of the workgroup is here, every sweep
            const uint32_t all = mine[0] | mine[1] | mine[2] | mine[3];
            any_changed = (all & 1u) != 0u;
            any_far = (all & 2u) != 0u;
        }
        cur ^= 1;
        if (!any_changed || !any_far || k == a.sweeps) break;   // the same answer in every thread of the problem
    }

    // Q_k of the last sweep from V_(k-1), which the other buffer still holds
    const float* const vo = vbuf + (cur ^ 1) * SP;
#pragma unroll
    for (int j = 0; j < CPL; ++j) {
        const int s = t + j * TPP;
        if (s < S) {
            float q[4];
            const float v = evaluate_cell(a, desc[j], prob[j], s, vo, q);
            if (a.q_out) a.q_out[base + s] = make_float4(q[0], q[1], q[2], q[3]);
            if (a.v_out) a.v_out[base + s] = v;
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

struct EvaluateFamily {
    using Args = EvaluateArgs;
    template <int VARIANT, int CPL, bool WAVE>
    static constexpr auto kernel() { return &evaluate_kernel<VARIANT, CPL, WAVE>; }
};
hipError_t launch_evaluate(int variant, const EvaluateArgs& a, hipStream_t s) { return launch_problems<EvaluateFamily>(variant, a, s); }

}  // namespace lmaze
