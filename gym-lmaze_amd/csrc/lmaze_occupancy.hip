// lmaze_occupancy.hip -- the discounted state occupancy of a table on the grid mazes (lmaze_occupancy / lmaze_describe_occupancy,
// include/lmaze.h): where the policy lmaze_evaluate values spends its discounted time, given where episodes start.  The adjoint
// of lmaze_evaluate.hip: that sweeps V <- r + gamma P V backward from the rewards, this sweeps D <- start + gamma P^T D forward
// from the start distribution, over the same model and the same four probabilities per cell.
//
// One problem = one maze of S = G*G states and one table, opened by lmaze_problem_frame.h as the other three families: sixteen
// model bits per cell in a register of the lane that owns the cell, the probabilities from evaluate_probs (lmaze_policy_probs.h).
// The transpose makes a cell gather: mass arrives over action a from the one cell c - step(a), with THAT cell's probability.
// The probabilities of a cell are its owner's, so they are exchanged once, at set-up, through the second buffer the frame
// leaves free: four rounds, one per action, each "owners write their masked p_a, sync, owners read their source's, sync".
// After that a cell keeps in registers its descriptor, the four incoming weights, the weight of the mass that stays (wall bumps
// and clamped targets) and its start mass -- seven words, 112 at sixteen cells per lane -- and a sweep makes the five LDS reads
// per cell that evaluate_kernel's makes, in an LDS of plan_solve's size.  The own probabilities are not kept: d_sa needs them
// once, after the last sweep, and reads the table again there.
//
// The sweep loop, the votes, the delta and the exit every thread of a problem takes in the same sweep are evaluate_kernel's.
#include <limits.h>
#include <math.h>
#include <stdio.h>

#include "lmaze_common.h"
#include "lmaze_learn.h"
#include "lmaze_policy_probs.h"
#include "lmaze_solve_model.h"

namespace lmaze {

// whether the pair's mass moves on: usable, not terminal (a terminal pair absorbs its mass, an excluded pair carries none)
__device__ __forceinline__ bool occupancy_flows(uint32_t nib) { return (nib & 3u) != SOLVE_EXCLUDED && !(nib & SOLVE_TERMINAL); }

// D_k(c) = start(c) + gamma * (sum_a win[a] * D_(k-1)(c - step(a)) + wself * D_(k-1)(c)): in the order a = 0..3, then the cell
// itself, from 0, over the weights that are not 0; every product and sum rounded on its own
__device__ __forceinline__ float occupancy_cell(int G, float gamma, uint32_t d, const float (&win)[4], float wself, float start,
                                                int s, const float* vo, float old) {
#pragma clang fp contract(off)
    if (d & SOLVE_WALL_STATE) return 0.0f;
    float acc = 0.0f;
#pragma unroll
    for (int act = 0; act < 4; ++act) {
        const int step = act == 0 ? -G : (act == 1 ? G : (act == 2 ? -1 : 1));
        const float from = vo[win[act] != 0.0f ? s - step : s];   // a weight that is 0 has no source on the grid to read
        if (win[act] != 0.0f) {
            const float term = win[act] * from;
            acc = acc + term;
        }
    }
    if (wself != 0.0f) {
        const float term = wself * old;
        acc = acc + term;
    }
    const float discounted = gamma * acc;
    return start + discounted;
}

// Seven words per cell: 112 registers at sixteen cells per lane against evaluate_kernel's 80, still inside the 256 that two
// waves per SIMD leave each, without scratch.
template <int VARIANT, int CPL, bool WAVE>
__global__ __launch_bounds__(LMAZE_BLOCK, (CPL == 16 ? 2 : 1)) void occupancy_kernel(const OccupancyArgs a) {
    extern __shared__ __align__(16) unsigned char occupancy_lds[];
    float win[CPL][4], wself[CPL], start[CPL];
    float prob[CPL][4];   // the cell's own: live through the set-up only
#define PROBLEM_LDS occupancy_lds
#define PROBLEM_WORD float
#define PROBLEM_AT_COPY(s) buf[s] = a.d_init ? a.d_init[base + s] : 0.0f   // D_0 goes into the first buffer
#define PROBLEM_AT_CELL(j) prob[j][0] = prob[j][1] = prob[j][2] = prob[j][3] = 0.0f   // like a wall state: no probabilities
#define PROBLEM_AT_DESC(j, s, d) evaluate_probs(a, base + s, d, prob[j])
#include "lmaze_problem_frame.h"
    // Set-up: what stays, the start mass, and the exchange of the probabilities that move
    float* const xbuf = buf + SP;
#pragma unroll
    for (int j = 0; j < CPL; ++j) {
        const int s = t + j * TPP;
        const bool free_cell = s < S && !(desc[j] & SOLVE_WALL_STATE);
        start[j] = free_cell ? a.start[base + s] : 0.0f;
        float w = 0.0f;
        bool first = true;
#pragma unroll
        for (int act = 0; act < 4; ++act) {
            const uint32_t nib = (desc[j] >> (4 * act)) & 15u;
            if (free_cell && occupancy_flows(nib) && !(nib & SOLVE_MOVED)) {
#pragma clang fp contract(off)
                const float sum = w + prob[j][act];
                w = first ? prob[j][act] : sum;
                first = false;
            }
        }
        wself[j] = w;
    }
#pragma unroll
    for (int act = 0; act < 4; ++act) {
        const int step = act == 0 ? -G : (act == 1 ? G : (act == 2 ? -1 : 1));
#pragma unroll
        for (int j = 0; j < CPL; ++j) {
            const int s = t + j * TPP;
            const uint32_t nib = (desc[j] >> (4 * act)) & 15u;
            if (s < S) xbuf[s] = (!(desc[j] & SOLVE_WALL_STATE) && occupancy_flows(nib) && (nib & SOLVE_MOVED)) ? prob[j][act] : 0.0f;
        }
        solve_sync<WAVE>();
#pragma unroll
        for (int j = 0; j < CPL; ++j) {
            const int s = t + j * TPP;
            float w = 0.0f;
            if (s < S && !(desc[j] & SOLVE_WALL_STATE)) {
                // the source cell c - step(a) by its coordinates: on the grid, and for a = 2, 3 in the same row
                const int x = s / G, y = s - x * G;
                const bool on = act == 0 ? x + 1 < G : (act == 1 ? x >= 1 : (act == 2 ? y + 1 < G : y >= 1));
                if (on) w = xbuf[s - step];
            }
            win[j][act] = w;
        }
        solve_sync<WAVE>();        // the round's words are read: the second buffer is free again
    }
    float* const vbuf = buf;

    // tol as a bit pattern: deltas are non-negative floats or NaNs, which order as unsigned integers with every NaN on top
    const bool use_tol = a.tol > 0.0f;
    const uint32_t tol_bits = __float_as_uint(a.tol);
    int cur = 0, k = 0;                // D_(k-1) is vbuf[cur]
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
                const float old = vo[s];
                const float v = occupancy_cell(G, a.gamma, desc[j], win[j], wself[j], start[j], s, vo, old);
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
            __syncthreads();           // D_k and the four votes; every thread of the workgroup is here, every sweep
            const uint32_t all = mine[0] | mine[1] | mine[2] | mine[3];
            any_changed = (all & 1u) != 0u;
            any_far = (all & 2u) != 0u;
        }
        cur ^= 1;
        if (!any_changed || !any_far || k == a.sweeps) break;   // the same answer in every thread of the problem
    }

    // D_k stands in vbuf[cur]; a cell's own word, which its owner wrote
    const float* const vk = vbuf + cur * SP;
#pragma unroll
    for (int j = 0; j < CPL; ++j) {
        const int s = t + j * TPP;
        if (s < S) {
            const float dk = vk[s];
            if (a.d_out) a.d_out[base + s] = dk;
            if (a.dsa_out) {
#pragma clang fp contract(off)
                float pr[4];
                evaluate_probs(a, base + s, desc[j], pr);   // the table again, once: not kept through the sweeps
                a.dsa_out[base + s] = make_float4(dk * pr[0], dk * pr[1], dk * pr[2], dk * pr[3]);
            }
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

struct OccupancyFamily {
    using Args = OccupancyArgs;
    template <int VARIANT, int CPL, bool WAVE>
    static constexpr auto kernel() { return &occupancy_kernel<VARIANT, CPL, WAVE>; }
};
hipError_t launch_occupancy(int variant, const OccupancyArgs& a, hipStream_t s) { return launch_problems<OccupancyFamily>(variant, a, s); }

}  // namespace lmaze
