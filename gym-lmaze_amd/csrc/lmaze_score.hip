// lmaze_score.hip -- what a table is worth on the grid mazes (lmaze_score / lmaze_describe_score, include/lmaze.h): the fewest
// steps to done from every cell, and the length of the walk that takes the table's action in every cell.
//
// One problem = one maze of S = G*G states and one deterministic table.  The model is solve_kernel's, from the function it
// uses (solve_descriptor over transition_rule, lmaze_solve_model.h): sixteen bits per cell, kept with the cell's action in a
// register by the lane that owns the cell.  A problem lives in LDS from its layout bytes to its results, in the two buffers of
// S words that solve_kernel keeps its values in, and the plan is plan_solve's: a wave per problem while S <= 256 (four per
// workgroup, no workgroup barrier), a workgroup per problem above.
//   distances     Jacobi min-plus sweeps between the two buffers, d(s) = 1 on a usable terminal pair, else 1 + the least d of
//                 the cells its usable pairs lead to.  d only falls, sweep k settles every distance <= k + 1, and the sweep
//                 that changes nothing ends them; at most S sweeps, a bound fixed before the loop.
//   walk lengths  pointer doubling between the same two buffers.  A word holds where the walk stands after 2^k steps in its
//                 upper half and the steps it took in its lower half; two values of the upper half that are no state stand for
//                 "arrived" (the lower half is then the answer) and "never", and absorb.  Round k reads the word of the cell a
//                 word points at and adds the halves: never in place, so a length is a sum of two lengths of the round before,
//                 at most 2^(k+1).  An arriving walk visits distinct cells, fewer than S of them, so after ceil(log2 S) rounds
//                 a pointer that is still a state belongs to a walk that never arrives.  That is the trip count, fixed before
//                 the loop; a round after which no pointer is a state ends it sooner.
// Every number is an integer and the result of a fixed point or of a fixed count of rounds, so no schedule changes it.  No loop
// waits for another wave: a mistake writes wrong numbers and returns.
#include <limits.h>
#include <stdio.h>

#include "lmaze_common.h"
#include "lmaze_learn.h"
#include "lmaze_solve_model.h"

namespace lmaze {

#define SCORE_INF 0x3FFFFFFF          // no terminal pair reached (yet): 1 + SCORE_INF is still an int32 and still above it
#define SCORE_ARRIVED 0xFFFFu         // upper half of a walk word: done was set, the lower half holds after how many steps
#define SCORE_NEVER 0xFFFEu           // upper half of a walk word: the walk never sets done; below both: a state, S <= 4096
#define SCORE_ACT_SHIFT 24            // the cell's action (a byte: above 3 is no action) over the descriptor's seventeen bits

__device__ __forceinline__ int score_step(int act, int G) { return act == 0 ? -G : (act == 1 ? G : (act == 2 ? -1 : 1)); }

// d_0: 1 on a usable terminal pair (a wall state's four nibbles are 0: none)
__device__ __forceinline__ int score_first(uint32_t d) {
    bool term = false;
#pragma unroll
    for (int act = 0; act < 4; ++act) {
        const uint32_t nib = (d >> (4 * act)) & 15u;
        term |= (nib & 3u) != SOLVE_EXCLUDED && (nib & SOLVE_TERMINAL);
    }
    return term ? 1 : SCORE_INF;
}

// d_k(s) from d_(k-1): a bump leads to the cell itself, which never lowers it
__device__ __forceinline__ int score_relax(uint32_t d, int s, int G, const int* dold) {
    int best = SCORE_INF;
#pragma unroll
    for (int act = 0; act < 4; ++act) {
        const uint32_t nib = (d >> (4 * act)) & 15u;
        const int dn = (nib & SOLVE_TERMINAL) ? 0 : dold[(nib & SOLVE_MOVED) ? s + score_step(act, G) : s];
        if ((nib & 3u) != SOLVE_EXCLUDED) best = min(best, dn + 1);
    }
    return best;
}

// the walk after one step: arrived, never (a wall state, no action, an excluded pair, a bump: a cycle of one), or the next cell
__device__ __forceinline__ uint32_t score_first_word(uint32_t d, int s, int G) {
    const uint32_t act = d >> SCORE_ACT_SHIFT;
    if ((d & SOLVE_WALL_STATE) || act > 3u) return SCORE_NEVER << 16;
    const uint32_t nib = (d >> (4 * act)) & 15u;
    if ((nib & 3u) == SOLVE_EXCLUDED) return SCORE_NEVER << 16;
    if (nib & SOLVE_TERMINAL) return (SCORE_ARRIVED << 16) | 1u;
    if (!(nib & SOLVE_MOVED)) return SCORE_NEVER << 16;
    return ((uint32_t)(s + score_step((int)act, G)) << 16) | 1u;
}

template <bool WAVE>
__device__ __forceinline__ bool score_vote(bool mine, uint32_t* vote, int& tick, int lane, int wave) {
    bool any = __ballot(mine) != 0ull;
    if constexpr (WAVE) {
        solve_sync<true>();
    } else {
        uint32_t* const w = vote + (tick & 1) * 4;
        ++tick;
        if (lane == 0) w[wave] = any ? 1u : 0u;
        __syncthreads();               // the buffer just written and the four votes; every thread of the workgroup is here
        any = (w[0] | w[1] | w[2] | w[3]) != 0u;
    }
    return any;
}

template <int VARIANT, int CPL, bool WAVE>
__global__ __launch_bounds__(LMAZE_BLOCK) void score_kernel(const ScoreArgs a) {
    extern __shared__ __align__(16) unsigned char score_lds[];
#define PROBLEM_LDS score_lds
#define PROBLEM_WORD int
#define PROBLEM_LOCALS const bool table = a.policy || a.q
#define PROBLEM_AT_COPY(s)
#define PROBLEM_BEFORE_SYNC if (!WAVE && threadIdx.x < 4) vote[8 + threadIdx.x] = 0u   // the four sums of the summary
#define PROBLEM_AT_DESC(j, s, d)                                                                     \
    uint32_t act = 0;                                                                                \
    if (a.q) {                                                                                       \
        const float4 row = a.q[base + s]; /* one 128-bit load per state */                           \
        const float r[4] = {row.x, row.y, row.z, row.w};                                             \
        int first;                                                                                   \
        lmaze_q_first_max(r, &first);                                                                \
        act = (uint32_t)first;                                                                       \
    } else if (a.policy) {                                                                           \
        act = a.policy[base + s];                                                                    \
    }                                                                                                \
    d |= act << SCORE_ACT_SHIFT
#include "lmaze_problem_frame.h"

    // ---- distances: d_0 into the first buffer, then sweeps
    int tick = 0, cur = 0;             // d_(k-1) is buf[cur]
#pragma unroll
    for (int j = 0; j < CPL; ++j) {
        const int s = t + j * TPP;
        if (s < S) buf[s] = score_first(desc[j]);
    }
    solve_sync<WAVE>();
    for (int k = 0; k < S; ++k) {
        const int* const dold = buf + cur * SP;
        int* const dnew = buf + (cur ^ 1) * SP;
        bool changed = false;
#pragma unroll
        for (int j = 0; j < CPL; ++j) {
            const int s = t + j * TPP;
            if (s < S) {
                const int d = score_relax(desc[j], s, G, dold);
                changed |= d != dold[s];
                dnew[s] = d;
            }
        }
        cur ^= 1;
        if (!score_vote<WAVE>(changed, vote, tick, lane, wave)) break;   // the same answer in every thread of the problem
    }
    int opt[CPL];
#pragma unroll
    for (int j = 0; j < CPL; ++j) {
        const int s = t + j * TPP;
        opt[j] = s < S ? buf[cur * SP + s] : SCORE_INF;
    }

    // ---- walk lengths: the word after one step into the other buffer (the last sweep's reads of it lie behind its vote),
    // then the doubling rounds; the first of them writes over the distances, which every thread holds in registers by then
    uint32_t* const wbuf = reinterpret_cast<uint32_t*>(buf);
    int src = cur ^ 1;
    if (table) {
#pragma unroll
        for (int j = 0; j < CPL; ++j) {
            const int s = t + j * TPP;
            if (s < S) wbuf[src * SP + s] = score_first_word(desc[j], s, G);
        }
        solve_sync<WAVE>();
        const int rounds = 32 - __clz(S - 1);       // ceil(log2 S): 2^rounds >= S
        for (int k = 0; k < rounds; ++k) {
            const uint32_t* const wo = wbuf + src * SP;
            uint32_t* const wn = wbuf + (src ^ 1) * SP;
            bool live = false;
#pragma unroll
            for (int j = 0; j < CPL; ++j) {
                const int s = t + j * TPP;
                if (s < S) {
                    uint32_t w = wo[s];
                    if ((w >> 16) < SCORE_NEVER) {
                        const uint32_t w2 = wo[w >> 16], to = w2 >> 16;
                        w = to == SCORE_NEVER ? SCORE_NEVER << 16 : (to << 16) | ((w & 0xFFFFu) + (w2 & 0xFFFFu));
                        live |= to < SCORE_NEVER;
                    }
                    wn[s] = w;
                }
            }
            src ^= 1;
            if (!score_vote<WAVE>(live, vote, tick, lane, wave)) break;
        }
    }

    // ---- results
    int reachable = 0, arrived = 0, shortest = 0, excess = 0;
#pragma unroll
    for (int j = 0; j < CPL; ++j) {
        const int s = t + j * TPP;
        if (s < S) {
            const int o = opt[j] >= SCORE_INF ? -1 : opt[j];
            int st = -1;
            if (table) {
                const uint32_t w = wbuf[src * SP + s];
                if ((w >> 16) == SCORE_ARRIVED) st = (int)(w & 0xFFFFu);
            }
            if (a.optimal) a.optimal[base + s] = o;
            if (a.steps) a.steps[base + s] = st;
            reachable += o >= 1;
            arrived += st >= 1;
            shortest += st >= 1 && st == o;
            excess += st >= 1 ? st - o : 0;
        }
    }
    if (a.summary) {
        reachable = wave_sum(reachable);
        arrived = wave_sum(arrived);
        shortest = wave_sum(shortest);
        excess = wave_sum(excess);
        if constexpr (!WAVE) {
            uint32_t* const sum = vote + 8;        // integer sums: their order changes nothing
            if (lane == 0) {
                atomicAdd(sum + 0, (uint32_t)reachable);
                atomicAdd(sum + 1, (uint32_t)arrived);
                atomicAdd(sum + 2, (uint32_t)shortest);
                atomicAdd(sum + 3, (uint32_t)excess);
            }
            __syncthreads();
            reachable = (int)sum[0];
            arrived = (int)sum[1];
            shortest = (int)sum[2];
            excess = (int)sum[3];
        }
        if (t == 0) {
            int32_t* const out = a.summary + p * 4;
            out[0] = reachable;
            out[1] = arrived;
            out[2] = shortest;
            out[3] = excess;
        }
    }
}

struct ScoreFamily {
    using Args = ScoreArgs;
    template <int VARIANT, int CPL, bool WAVE>
    static constexpr auto kernel() { return &score_kernel<VARIANT, CPL, WAVE>; }
};
hipError_t launch_score(int variant, const ScoreArgs& a, hipStream_t s) { return launch_problems<ScoreFamily>(variant, a, s); }

}  // namespace lmaze
