// lmaze_rollout_body.h -- the bodies of the three v0/v3 rollout kernels of lmaze_step.hip, each included into the plain
// form (RolloutArgs, REC false) and the recording form (RolloutObsArgs, REC true) of its kernel: through a __device__
// function the plain forms compiled to other register allocations, included they keep their code.  In scope: `a`
// (StepArgs), `ro`, the compile-time VARIANT, REC and, for the wave-autonomous body, EPW.  LMAZE_ROLLOUT_BODY selects
// the body: 1 rollout_shared_wave8_kernel, 2 rollout_shared_kernel, 3 rollout_perenv_kernel, 4 rollout_shared_u8_kernel
// (whose recording form takes RolloutObs8Args).  With LMAZE_ROLLOUT_POLICY defined, bodies 2-4 are the closed-loop forms
// (RolloutPolicyArgs, u8: RolloutPolicy8Args; REC true): no action row is read -- after the fused reset the lane that owns
// the env looks its action up by the env's key (policy_act) -- and the ball-keyed table sits in LDS behind the body's other
// arrays.  The lines of the open-loop forms are the #else branches, untouched.  LMAZE_ROLLOUT_POLICY == 2: the sampling
// forms (RolloutSampleArgs, u8: RolloutSample8Args) -- the same lines, but the table holds one sample_row_t of thresholds per key.
// LMAZE_ROLLOUT_POLICY == 3 / 4, bodies 2 and 3: the epsilon-greedy / sampling forms with a table PER ENV (RolloutEnvBytesArgs /
// RolloutEnvRowsArgs): `tab` is the lane's pointer to its own env's rows -- in LDS for body 3's byte tables, staged behind the
// layouts (LMAZE_TAB_ENV_BYTES), in global memory everywhere else.  LMAZE_ROLLOUT_POLICY == 5, bodies 2 and 3: the Q-learner
// (RolloutEnvQArgs): `tab` is the lane's QLane -- its env's rows in global memory, the cell policy_act looked up and the row carried
// from the step before -- and after the transition qlearn_update writes that cell's row back.
// Where each array of bodies 2-4 lies in LDS is lmaze_rollout_lds.h's to say, the text the host sizes the launch from (L; the
// table by the form's kind, which moves no other array).  Not a header of its own.
#ifndef LMAZE_ROLLOUT_BODY
#error "lmaze_rollout_body.h is the body of the rollout kernels: it is included only inside them, in lmaze_step.hip"
#endif
#if LMAZE_ROLLOUT_BODY == 1
    constexpr bool V3 = VARIANT == LMAZE_VARIANT_V3;
    constexpr int G = 8, CELLS = 64;
    const int lane = threadIdx.x & 63;
    const int64_t base = ((int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6)) * EPW;
    if (base >= a.n) return;
    const int nb = (int)min((int64_t)EPW, a.n - base);
    const bool autoreset = a.auto_reset != 0;
    const bool live = lane < nb;
    const int64_t e = base + lane;
    const int myc = a.layout[lane];
    EnvState s = rollout_load<VARIANT>(a, ro, e, live);
    int hits = 0, act_next = s.act;
    const int mypat = cell_bits<VARIANT>((uint8_t)myc);
    const int p4 = (lane & 15) << 2;
    const int4 pat4 = make_int4(__shfl(mypat, p4, 64), __shfl(mypat, p4 + 1, 64), __shfl(mypat, p4 + 2, 64),
                                __shfl(mypat, p4 + 3, 64));
    const unsigned long long ok[1] = {__ballot(interior(lane, G) && spawn_ok<VARIANT>((uint8_t)myc))};
    int4* obs4 = a.obs ? reinterpret_cast<int4*>(a.obs + (size_t)base * CELLS) : nullptr;
    for (int t = 0; t < ro.T; ++t) {
        s.act = act_next;
        if (t + 1 < ro.T && live) act_next = ro.actions[(size_t)(t + 1) * a.n + e];      // next step's row, in flight over this step
        if (autoreset && s.done) {   // as step_shared_wave8_kernel, with this step's epoch
            int bc, gc;
            place_from_masks<VARIANT, 1>(ok, __popcll(ok[0]), env_draw(a.seed, a.epoch + (uint64_t)t, a.env_base + e), bc, gc);
            env_reset<VARIANT>(bc, gc, G, s);
        }
        // every lane takes part in the __shfl
        hits += env_advance<VARIANT>(a, G, [&](int tx, int ty) { return (uint8_t)__shfl(myc, tx * G + ty, 64); }, s) ? 1 : 0;
        if (live) rollout_record(ro, a.n, t, e, s);
        if constexpr (!REC) {
            if (obs4) {
                const int ball_cell = ball_cell_of(s.b, G);
                const int goal_cell = goal_cell_of<VARIANT>(s.g, G);
#pragma unroll
                for (int k = 0; k < EPW / 4; ++k) {
                    const int le = (lane >> 4) + 4 * k;
                    const int bc = __shfl(ball_cell, le, 64);
                    const int gc = V3 ? __shfl(goal_cell, le, 64) : -8;
                    int4 v = pat4;
                    or_at(v, bc - p4, LMAZE_OBS_BALL);
                    if (V3) or_at(v, gc - p4, LMAZE_OBS_GOAL);
                    if (le < nb) obs4[lane + 64 * k] = v;
                }
            }
            continue;
        }
        // the slot this step fills (uniform over the wave) and, after the last step, the caller's planes: one render,
        // stored to both when both are due
        int4* dst = reinterpret_cast<int4*>(rollout_slot(ro, a.n, base, CELLS, t));
        int4* also = obs4 && t == ro.T - 1 ? obs4 : nullptr;
        if (dst == nullptr) { dst = also; also = nullptr; }
        if (dst) {
            const int ball_cell = ball_cell_of(s.b, G);
            const int goal_cell = goal_cell_of<VARIANT>(s.g, G);
#pragma unroll
            for (int k = 0; k < EPW / 4; ++k) {
                const int le = (lane >> 4) + 4 * k;
                const int bc = __shfl(ball_cell, le, 64);
                const int gc = V3 ? __shfl(goal_cell, le, 64) : -8;
                int4 v = pat4;
                or_at(v, bc - p4, LMAZE_OBS_BALL);
                if (V3) or_at(v, gc - p4, LMAZE_OBS_GOAL);
                if (le < nb) {
                    dst[lane + 64 * k] = v;
                    if (also) also[lane + 64 * k] = v;
                }
            }
        }
    }
    rollout_store<VARIANT>(a, ro, e, live, s, hits);
#elif LMAZE_ROLLOUT_BODY == 2
    constexpr bool V3 = VARIANT == LMAZE_VARIANT_V3;
    const int G = a.grid, CELLS = G * G, EPB = a.envs_per_block;
    extern __shared__ __attribute__((aligned(16))) char lds[];
    const LmazeRolloutLds L = lmaze_rollout_lds_shared(CELLS, EPB, LMAZE_TAB_NONE);
    int* pat = reinterpret_cast<int*>(lds + L.pat);                           // [CELLS] plane bits without ball / goal
    int* ballflat = reinterpret_cast<int*>(lds + L.ballflat);                 // [EPB]
    int* goalflat = reinterpret_cast<int*>(lds + L.goalflat);                 // [EPB]
    uint8_t* lay = reinterpret_cast<uint8_t*>(lds + L.lay);                   // [CELLS]
    uint16_t* spawn = reinterpret_cast<uint16_t*>(lds + L.spawn);             // [CELLS] accepted spawn cells, row-major
    __shared__ int spawn_count_s;

    const int tid = threadIdx.x;
    const int64_t blockbase = (int64_t)blockIdx.x * EPB;
    const int nb = (int)min((int64_t)EPB, a.n - blockbase);
    const bool autoreset = a.auto_reset != 0, live = tid < nb;
    const int64_t e = blockbase + tid;
#ifdef LMAZE_ROLLOUT_POLICY
#if LMAZE_ROLLOUT_POLICY == 2
    sample_row_t* tab = reinterpret_cast<sample_row_t*>(lds + lmaze_rollout_lds_shared(CELLS, EPB, LMAZE_TAB_ROWS).tab);   // [CELLS] staged thresholds
    EnvState s = policy_load<VARIANT>(a, e, live);                            // in flight over the set-up
    int hits = 0;
    if (ro.pol.staged)
        for (int i = tid; i < CELLS; i += LMAZE_BLOCK) tab[i] = ro.pol.table[i];      // 16-byte copies
#elif LMAZE_ROLLOUT_POLICY == 5
    // a Q table per env, read and written in global memory: the lane's rows and, from policy_act on, the step's cell
    QLane tab{env_table_global(ro.pol) + e * CELLS, 0, {}, -1, {}};           // next_cell -1: no row carried yet
    EnvState s = policy_load<VARIANT>(a, e, live);                            // in flight over the set-up
    int hits = 0;
#elif LMAZE_ROLLOUT_POLICY >= 3
    // a table per env, left in global memory: the lane's pointer to its env's own rows (without an env: formed, never followed)
    const auto tab = env_table_global(ro.pol) + e * CELLS;
    EnvState s = policy_load<VARIANT>(a, e, live);                            // in flight over the set-up
    int hits = 0;
#else
    uint8_t* tab = reinterpret_cast<uint8_t*>(lds + lmaze_rollout_lds_shared(CELLS, EPB, LMAZE_TAB_BYTES).tab);   // [CELLS] the ball-keyed table
    EnvState s = policy_load<VARIANT>(a, e, live);                            // in flight over the set-up
    int hits = 0;
    if (ro.pol.key_mode == 0)
        for (int i = tid; i < CELLS; i += LMAZE_BLOCK) tab[i] = ro.pol.table[i];
#endif
#else
    EnvState s = rollout_load<VARIANT>(a, ro, e, live);                       // in flight over the set-up
    int hits = 0, act_next = s.act;
#endif
    for (int i = tid; i < CELLS; i += LMAZE_BLOCK) {
        const uint8_t c = a.layout[i];
        lay[i] = c;
        pat[i] = cell_bits<VARIANT>(c);
    }
    if (autoreset && tid < 64) {
        const int cnt = wave_build_spawn_list<VARIANT>(a.layout, G, CELLS, spawn, tid);
        if (tid == 0) spawn_count_s = cnt;
    }
    __syncthreads();
    const int spawn_count = autoreset ? spawn_count_s : 0;

    int32_t* obs = a.obs ? a.obs + (size_t)blockbase * CELLS : nullptr;
    for (int t = 0; t < ro.T; ++t) {
        if (live) {
#ifndef LMAZE_ROLLOUT_POLICY
            s.act = act_next;
            if (t + 1 < ro.T) act_next = ro.actions[(size_t)(t + 1) * a.n + e];       // next step's row, in flight over this step
#endif
            if (autoreset && s.done) {                                                // as env_phase1
                int bc, gc;
                place_from_list<VARIANT>(spawn, spawn_count, env_draw(a.seed, a.epoch + (uint64_t)t, a.env_base + e), bc, gc);
                env_reset<VARIANT>(bc, gc, G, s);
            }
#ifdef LMAZE_ROLLOUT_POLICY
            policy_act<VARIANT>(a, ro.pol, tab, G, t, e, s);                          // the action of the state just reset
#endif
            hits += env_advance<VARIANT>(a, G, [&](int tx, int ty) { return lay[tx * G + ty]; }, s) ? 1 : 0;
#if defined(LMAZE_ROLLOUT_POLICY) && LMAZE_ROLLOUT_POLICY == 5
            qlearn_update(ro.pol, tab, G, a.n, t, e, s);                              // learns from what the step returned
#endif
            rollout_record(ro, a.n, t, e, s);
            ballflat[tid] = ball_cell_of(s.b, G);
            if (V3) goalflat[tid] = goal_cell_of<VARIANT>(s.g, G);
        }
        if constexpr (REC) {
            int32_t* slot = rollout_slot(ro, a.n, blockbase, CELLS, t);
            int32_t* last = t == ro.T - 1 ? obs : nullptr;
            if (slot == nullptr && last == nullptr) continue;                         // uniform: nothing recorded
            __syncthreads();
            if (slot) rollout_render<VARIANT>(slot, nb * CELLS, CELLS, ballflat, goalflat, [&](int, int c) { return pat[c]; }, slot_nt(ro));
            if (last) rollout_render<VARIANT>(last, nb * CELLS, CELLS, ballflat, goalflat, [&](int, int c) { return pat[c]; });
            __syncthreads();
            continue;
        }
        if (obs == nullptr) continue;                                                 // uniform
        __syncthreads();
        rollout_render<VARIANT>(obs, nb * CELLS, CELLS, ballflat, goalflat, [&](int, int c) { return pat[c]; });
        __syncthreads();                                                              // ballflat / goalflat are rewritten by the next step
    }
    rollout_store<VARIANT>(a, ro, e, live, s, hits);
#elif LMAZE_ROLLOUT_BODY == 3
    constexpr bool V3 = VARIANT == LMAZE_VARIANT_V3;
    const int G = a.grid, CELLS = G * G, EPB = a.envs_per_block;
    extern __shared__ __attribute__((aligned(16))) char lds[];
    const LmazeRolloutLds L = lmaze_rollout_lds_perenv(CELLS, EPB, LMAZE_TAB_NONE);
    int* ballflat = reinterpret_cast<int*>(lds + L.ballflat);                 // [EPB] cell of the ball
    int* goalflat = reinterpret_cast<int*>(lds + L.goalflat);                 // [EPB]
    uint8_t* lays = reinterpret_cast<uint8_t*>(lds + L.lay);                  // [EPB * CELLS]

    const int tid = threadIdx.x;
    const int64_t blockbase = (int64_t)blockIdx.x * EPB;
    const int nb = (int)min((int64_t)EPB, a.n - blockbase);
    const bool autoreset = a.auto_reset != 0, live = tid < nb;
    const int64_t e = blockbase + tid;
#ifdef LMAZE_ROLLOUT_POLICY
#if LMAZE_ROLLOUT_POLICY == 2
    sample_row_t* tab = reinterpret_cast<sample_row_t*>(lds + lmaze_rollout_lds_perenv(CELLS, EPB, LMAZE_TAB_ROWS).tab);   // [CELLS] staged thresholds
    EnvState s = policy_load<VARIANT>(a, e, live);
    int hits = 0;
    if (ro.pol.staged)
        for (int i = tid; i < CELLS; i += LMAZE_BLOCK) tab[i] = ro.pol.table[i];      // 16-byte copies
#elif LMAZE_ROLLOUT_POLICY == 3
    // a byte table per env, staged below behind the layouts and by their copy: [EPB * CELLS], env tid's rows at tid * CELLS
    uint8_t* tabs = reinterpret_cast<uint8_t*>(lds + lmaze_rollout_lds_perenv(CELLS, EPB, LMAZE_TAB_ENV_BYTES).tab);
    const env_bytes_lds tab = (env_bytes_lds)tabs + tid * CELLS;
    EnvState s = policy_load<VARIANT>(a, e, live);
    int hits = 0;
#elif LMAZE_ROLLOUT_POLICY == 4
    // a threshold table per env, 16 bytes per cell: left in global memory, the lane's pointer to its env's own rows
    const auto tab = env_table_global(ro.pol) + e * CELLS;
    EnvState s = policy_load<VARIANT>(a, e, live);
    int hits = 0;
#elif LMAZE_ROLLOUT_POLICY == 5
    // a Q table per env, read and written in global memory: the lane's rows and, from policy_act on, the step's cell
    QLane tab{env_table_global(ro.pol) + e * CELLS, 0, {}, -1, {}};
    EnvState s = policy_load<VARIANT>(a, e, live);
    int hits = 0;
#else
    uint8_t* tab = reinterpret_cast<uint8_t*>(lds + lmaze_rollout_lds_perenv(CELLS, EPB, LMAZE_TAB_BYTES).tab);   // [CELLS] the ball-keyed table
    EnvState s = policy_load<VARIANT>(a, e, live);
    int hits = 0;
    if (ro.pol.key_mode == 0)
        for (int i = tid; i < CELLS; i += LMAZE_BLOCK) tab[i] = ro.pol.table[i];
#endif
#else
    EnvState s = rollout_load<VARIANT>(a, ro, e, live);
    int hits = 0, act_next = s.act;
#endif
    {   // EPB is a multiple of 4: the workgroup's layouts start on a dword and are whole dwords
        const uint32_t* src = reinterpret_cast<const uint32_t*>(a.layout + (size_t)blockbase * CELLS);
        uint32_t* dst = reinterpret_cast<uint32_t*>(lays);
        const int nw = (nb * CELLS) >> 2;
        for (int i = tid; i < nw; i += LMAZE_BLOCK) dst[i] = src[i];
        for (int i = (nw << 2) + tid; i < nb * CELLS; i += LMAZE_BLOCK) lays[i] = a.layout[(size_t)blockbase * CELLS + i];
#if defined(LMAZE_ROLLOUT_POLICY) && LMAZE_ROLLOUT_POLICY == 3
        // the same for the workgroup's tables: same offset, and the ABI has checked the table's base for a dword
        const uint32_t* tsrc = reinterpret_cast<const uint32_t*>(ro.pol.table + (size_t)blockbase * CELLS);
        uint32_t* tdst = reinterpret_cast<uint32_t*>(tabs);
        for (int i = tid; i < nw; i += LMAZE_BLOCK) tdst[i] = tsrc[i];
        for (int i = (nw << 2) + tid; i < nb * CELLS; i += LMAZE_BLOCK) tabs[i] = ro.pol.table[(size_t)blockbase * CELLS + i];
#endif
    }
    __syncthreads();

    int32_t* obs = a.obs ? a.obs + (size_t)blockbase * CELLS : nullptr;
    for (int t = 0; t < ro.T; ++t) {
        if (tid < 64) {                                                               // wave 0, every lane: the ballots below
#ifndef LMAZE_ROLLOUT_POLICY
            s.act = act_next;
            if (live && t + 1 < ro.T) act_next = ro.actions[(size_t)(t + 1) * a.n + e];
#endif
            // reference reset() of the done envs, one whole-wave placement each on the env's own layout
            unsigned long long todo = __ballot(live && autoreset && s.done);
            while (todo) {
                const int j = __ffsll((long long)todo) - 1;
                todo &= todo - 1ull;
                int bc, gc;
                wave_place<VARIANT>(lays + j * CELLS, G, CELLS, env_draw(a.seed, a.epoch + (uint64_t)t, a.env_base + blockbase + j), tid, bc, gc);
                if (tid == j) env_reset<VARIANT>(bc, gc, G, s);
            }
            if (live) {
#ifdef LMAZE_ROLLOUT_POLICY
                policy_act<VARIANT>(a, ro.pol, tab, G, t, e, s);                      // the action of the state just reset
#endif
                hits += env_advance<VARIANT>(a, G, [&](int tx, int ty) { return lays[tid * CELLS + tx * G + ty]; }, s) ? 1 : 0;
#if defined(LMAZE_ROLLOUT_POLICY) && LMAZE_ROLLOUT_POLICY == 5
                qlearn_update(ro.pol, tab, G, a.n, t, e, s);                          // learns from what the step returned
#endif
                rollout_record(ro, a.n, t, e, s);
                ballflat[tid] = ball_cell_of(s.b, G);
                if (V3) goalflat[tid] = goal_cell_of<VARIANT>(s.g, G);
            }
        }
        if constexpr (REC) {
            auto bits = [&](int le, int c) { return cell_bits<VARIANT>(lays[le * CELLS + c]); };
            int32_t* slot = rollout_slot(ro, a.n, blockbase, CELLS, t);
            int32_t* last = t == ro.T - 1 ? obs : nullptr;
            if (slot == nullptr && last == nullptr) continue;                         // uniform: nothing recorded
            __syncthreads();
            if (slot) rollout_render<VARIANT>(slot, nb * CELLS, CELLS, ballflat, goalflat, bits, slot_nt(ro));
            if (last) rollout_render<VARIANT>(last, nb * CELLS, CELLS, ballflat, goalflat, bits);
            __syncthreads();
            continue;
        }
        if (obs == nullptr) continue;                                                 // uniform
        __syncthreads();
        rollout_render<VARIANT>(obs, nb * CELLS, CELLS, ballflat, goalflat,
                                [&](int le, int c) { return cell_bits<VARIANT>(lays[le * CELLS + c]); });
        __syncthreads();
    }
    rollout_store<VARIANT>(a, ro, e, live, s, hits);
#elif LMAZE_ROLLOUT_BODY == 4
    // body 2 with the narrow planes of step_shared_u8_kernel: the same set-up in LDS (layout, byte-shifted pattern copies,
    // spawn list), the same transition, and each step's render through rollout_render_u8
    constexpr bool V3 = VARIANT == LMAZE_VARIANT_V3;
    const int G = a.grid, CELLS = G * G, EPB = a.envs_per_block;
    const int PW = lmaze_rollout_u8_pw(CELLS);                                // dwords of one shifted copy, as step_shared_u8_kernel
    extern __shared__ __attribute__((aligned(16))) char lds[];
    const LmazeRolloutLds L = lmaze_rollout_lds_u8(CELLS, EPB, LMAZE_TAB_NONE);
    uint32_t* patw = reinterpret_cast<uint32_t*>(lds + L.pat);                // [4][PW] copy s = the doubled pattern from byte s
    int* ballflat = reinterpret_cast<int*>(lds + L.ballflat);                 // [EPB + 1]
    int* goalflat = reinterpret_cast<int*>(lds + L.goalflat);                 // [EPB + 1]
    uint16_t* spawn = reinterpret_cast<uint16_t*>(lds + L.spawn);             // [CELLS] accepted spawn cells, row-major
    uint8_t* lay = reinterpret_cast<uint8_t*>(lds + L.lay);                   // [CELLS]
    __shared__ int spawn_count_s;

    const int tid = threadIdx.x;
    const int64_t blockbase = (int64_t)blockIdx.x * EPB;
    const int nb = (int)min((int64_t)EPB, a.n - blockbase);
    const bool autoreset = a.auto_reset != 0, live = tid < nb;
    const int64_t e = blockbase + tid;
#ifdef LMAZE_ROLLOUT_POLICY
#if LMAZE_ROLLOUT_POLICY == 2
    sample_row_t* tab = reinterpret_cast<sample_row_t*>(lds + lmaze_rollout_lds_u8(CELLS, EPB, LMAZE_TAB_ROWS).tab);   // [CELLS] staged thresholds
    EnvState s = policy_load<VARIANT>(a, e, live);                            // in flight over the set-up
    int hits = 0;
    if (ro.pol.staged)
        for (int i = tid; i < CELLS; i += LMAZE_BLOCK) tab[i] = ro.pol.table[i];      // 16-byte copies
#else
    uint8_t* tab = reinterpret_cast<uint8_t*>(lds + lmaze_rollout_lds_u8(CELLS, EPB, LMAZE_TAB_BYTES).tab);   // [CELLS] the ball-keyed table
    EnvState s = policy_load<VARIANT>(a, e, live);                            // in flight over the set-up
    int hits = 0;
    if (ro.pol.key_mode == 0)
        for (int i = tid; i < CELLS; i += LMAZE_BLOCK) tab[i] = ro.pol.table[i];
#endif
#else
    EnvState s = rollout_load<VARIANT>(a, ro, e, live);                       // in flight over the set-up
    int hits = 0, act_next = s.act;
#endif
    for (int i = tid; i < CELLS; i += LMAZE_BLOCK) lay[i] = a.layout[i];
    for (int i = tid; i <= EPB; i += LMAZE_BLOCK) { ballflat[i] = -64; goalflat[i] = -64; }
    __syncthreads();
    for (int i = tid; i < 4 * PW; i += LMAZE_BLOCK) {                         // as step_shared_u8_kernel's set-up
        const int sc = i / PW, k = (i - sc * PW) << 2;
        uint32_t w = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            int c = k + sc + j;
            c -= c >= CELLS ? CELLS : 0;
            c -= c >= CELLS ? CELLS : 0;
            c = min(c, CELLS - 1);
            w |= (uint32_t)cell_bits<VARIANT>(lay[c]) << (8 * j);
        }
        patw[i] = w;
    }
    if (autoreset && tid < 64) {
        const int cnt = wave_build_spawn_list<VARIANT>(lay, G, CELLS, spawn, tid);
        if (tid == 0) spawn_count_s = cnt;
    }
    __syncthreads();
    const int spawn_count = autoreset ? spawn_count_s : 0;

    // EPB is a multiple of 16: the workgroup's range of obs8 starts on a 16-byte boundary (the ABI checks obs8's base)
    uint8_t* obs = a.obs8 ? a.obs8 + (size_t)blockbase * CELLS : nullptr;
    const int R = nb * CELLS;
    for (int t = 0; t < ro.T; ++t) {
        if (live) {
#ifndef LMAZE_ROLLOUT_POLICY
            s.act = act_next;
            if (t + 1 < ro.T) act_next = ro.actions[(size_t)(t + 1) * a.n + e];       // next step's row, in flight over this step
#endif
            if (autoreset && s.done) {                                                // as env_phase1
                int bc, gc;
                place_from_list<VARIANT>(spawn, spawn_count, env_draw(a.seed, a.epoch + (uint64_t)t, a.env_base + e), bc, gc);
                env_reset<VARIANT>(bc, gc, G, s);
            }
#ifdef LMAZE_ROLLOUT_POLICY
            policy_act<VARIANT>(a, ro.pol, tab, G, t, e, s);                          // the action of the state just reset
#endif
            hits += env_advance<VARIANT>(a, G, [&](int tx, int ty) { return lay[tx * G + ty]; }, s) ? 1 : 0;
            rollout_record(ro, a.n, t, e, s);
            ballflat[tid] = ball_cell_of(s.b, G);
            if (V3) goalflat[tid] = goal_cell_of<VARIANT>(s.g, G);
        }
        // the slot this step fills (recording form) and the caller's planes: every step in the plain form, as T step
        // launches would write them; after the last step only in the recording form
        uint8_t* slot = rollout_slot8(ro, a.n, blockbase, CELLS, t);
        uint8_t* last = (!REC || t == ro.T - 1) ? obs : nullptr;
        if (slot == nullptr && last == nullptr) continue;                             // uniform: nothing stored
        __syncthreads();
        if (slot) rollout_render_u8<VARIANT>(slot, R, CELLS, nb, patw, PW, ballflat, goalflat);
        if (last) rollout_render_u8<VARIANT>(last, R, CELLS, nb, patw, PW, ballflat, goalflat);
        __syncthreads();                                                              // ballflat / goalflat are rewritten by the next step
    }
    rollout_store<VARIANT>(a, ro, e, live, s, hits);
#endif
