// lmaze_problem_frame.h -- a problem from its indices to its descriptors: the opening lines of solve_kernel, score_kernel,
// evaluate_kernel and occupancy_kernel (lmaze_solve.hip, lmaze_score.hip, lmaze_evaluate.hip, lmaze_occupancy.hip), included
// into each as lmaze_rollout_body.h is into its kernels: through a __device__ function the kernels compiled to other register
// allocations, included they keep their code.
// In scope: `a` (SolveArgs, ScoreArgs, EvaluateArgs or OccupancyArgs: layouts, goal, problems, grid, per_env and the three
// rewards) and the compile-time VARIANT, CPL, WAVE.  The kernel defines
//   PROBLEM_LDS              its extern __shared__ bytes: per workgroup two buffers of SP words for each of its PPW problems,
//                            the StepArgs the rule is asked with, and the vote words (SOLVE_VOTE_BYTES, workgroup form only)
//   PROBLEM_WORD             what a buffer's word is to it (float, int)
//   PROBLEM_AT_COPY(s)       a statement beside the copy of cell s's layout byte (V_0 into the first buffer), s < S
//   PROBLEM_AT_DESC(j, s, d) a statement that may add to d, cell s's sixteen bits (solve_descriptor), or read a table by it, s < S
// and may define, each for a line that one kernel alone has there,
//   PROBLEM_LOCALS           a declaration behind the early return (score_kernel: whether it has a table)
//   PROBLEM_BEFORE_SYNC      a statement before the first sync, when vote stands (score_kernel clears its sums there)
//   PROBLEM_AT_CELL(j)       a statement for each of the lane's cells, s < S or not (evaluate_kernel, occupancy_kernel: no
//                            probabilities yet)
// and finds behind it TPP, PPW, SP, lane, wave, t, p, buf, vote, G, S, base and desc[CPL], the second buffer free again.  The
// hooks keep each kernel's global loads, and every other line of it, where they were between the syncs.  Not a header of its own.
#if !defined(PROBLEM_LDS) || !defined(PROBLEM_WORD) || !defined(PROBLEM_AT_COPY) || !defined(PROBLEM_AT_DESC)
#error "lmaze_problem_frame.h is the opening of the solve, score and evaluate kernels: it is included only inside them"
#endif
    constexpr int TPP = WAVE ? 64 : LMAZE_BLOCK;        // threads per problem
    constexpr int PPW = LMAZE_BLOCK / TPP;              // problems per workgroup
    constexpr int SP = CPL * TPP;                       // words of one buffer, >= S
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int t = WAVE ? lane : (int)threadIdx.x;
    const int64_t p = (int64_t)blockIdx.x * PPW + (WAVE ? wave : 0);
    // wave form: a whole wave without a problem, and no barrier in that form waits for it; workgroup form: never
    if (p >= a.problems) return;
    PROBLEM_WORD* const buf = reinterpret_cast<PROBLEM_WORD*>(PROBLEM_LDS) + (WAVE ? wave : 0) * 2 * SP;
    uint32_t* const vote = reinterpret_cast<uint32_t*>(PROBLEM_LDS + (size_t)PPW * 2 * SP * sizeof(PROBLEM_WORD) + SOLVE_MODEL_BYTES);   // workgroup form only
    const int G = a.grid, S = G * G;
    const int64_t base = p * S;
#ifdef PROBLEM_LOCALS
    PROBLEM_LOCALS;
#undef PROBLEM_LOCALS
#endif

    // the layout's bytes borrow the second buffer until the descriptors are built
    uint8_t* const lay = reinterpret_cast<uint8_t*>(buf + SP);
    const uint8_t* const lay_g = a.layouts + (a.per_env ? base : 0);
#pragma unroll
    for (int j = 0; j < CPL; ++j) {
        const int s = t + j * TPP;
        if (s < S) {
            lay[s] = lay_g[s];
            PROBLEM_AT_COPY(s);
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
    StepArgs* const m = reinterpret_cast<StepArgs*>(PROBLEM_LDS + (size_t)PPW * 2 * SP * sizeof(PROBLEM_WORD));
    if (lane == 0) {
        m->reward_wall = a.reward_wall;
        m->reward_move = a.reward_move;
        m->reward_goal = a.reward_goal;
        m->step_limit = INT_MAX;
    }
#ifdef PROBLEM_BEFORE_SYNC
    PROBLEM_BEFORE_SYNC;
#undef PROBLEM_BEFORE_SYNC
#endif
    solve_sync<WAVE>();
    uint32_t desc[CPL];
#pragma unroll
    for (int j = 0; j < CPL; ++j) {
        const int s = t + j * TPP;
        uint32_t d = SOLVE_WALL_STATE;
#ifdef PROBLEM_AT_CELL
        PROBLEM_AT_CELL(j);
#endif
        if (s < S) {
            d = solve_descriptor<VARIANT>(*m, lay, G, s, gx, gy);
            PROBLEM_AT_DESC(j, s, d);
        }
        desc[j] = d;
    }
    solve_sync<WAVE>();                // the layout's bytes are read: the second buffer is free
#undef PROBLEM_LDS
#undef PROBLEM_WORD
#undef PROBLEM_AT_COPY
#undef PROBLEM_AT_DESC
#undef PROBLEM_AT_CELL
