// lmaze_foveal_body.h -- the body of foveal_kernel and foveal_rollout_kernel (lmaze_foveal.hip), included into each.
// In scope: the kernel argument `a` (FovealArgs), `ro` (FovealRoll, or FovealRollObs), and the compile-time VARIANT, MODE,
// EPB, GT, AR, ROLL (the rollout: every chunk runs ro.T steps before the workgroup takes the next one), REC (the
// recording rollout: phases 3 and 3b also store the observations of every k-th step into the caller's slots) and POL (the
// closed-loop rollout of v1/v2/v4, lmaze_foveal_policy.hip: phase 1 takes the action from a table keyed by the env's state,
// mixed with an exploration draw, instead of from the action tensor, and stores the action and key rows).  POL is the
// include site's LMAZE_FOVEAL_POLICY_SITE: what it adds stands under the preprocessor, so that every other kernel compiles
// from the text it always had.  LMAZE_FOVEAL_SAMPLE_SITE (lmaze_foveal_sample.hip, POL = 2) is the sampling closed loop: the
// table holds one row of cumulative thresholds per key and one draw word is compared against them.
// LMAZE_FOVEAL_HIER_SITE (lmaze_hier_policy.hip, POL = 3) is the closed loop of the two-level step of v5/v6: the V5 FM_STEP / AR
// branch of phase 1 loads neither a.action nor a.goal2; the planner's goal and the controller's action come from two tables
// (ro.hier) mixed with one draw, and their rows are stored where they are produced.  LMAZE_FOVEAL_HIER_SAMPLE_SITE
// (lmaze_hier_sample.hip, POL = 4) is that loop's sampling form: both tables hold rows of cumulative thresholds (ro.hsmp), staged
// as POL 2 stages its one, and the words r.x and r.z of a draw taken on every env-step are compared against them.  Not a header
// of its own.
#ifndef LMAZE_FOVEAL_BODY_SITE
#error "lmaze_foveal_body.h is the body of the foveal kernels: it is included only inside them, in lmaze_foveal.hip, lmaze_foveal_policy.hip, lmaze_foveal_sample.hip, lmaze_hier_policy.hip and lmaze_hier_sample.hip"
#endif
#if defined(LMAZE_FOVEAL_HIER_SAMPLE_SITE)
#define LMAZE_POL 4
#elif defined(LMAZE_FOVEAL_HIER_SITE)
#define LMAZE_POL 3
#elif defined(LMAZE_FOVEAL_SAMPLE_SITE)
#define LMAZE_POL 2
#elif defined(LMAZE_FOVEAL_POLICY_SITE)
#define LMAZE_POL 1
#else
#define LMAZE_POL 0
#endif
    constexpr bool V1 = VARIANT == LMAZE_VARIANT_V1, V5 = VARIANT == LMAZE_VARIANT_V5;
    constexpr bool V4 = VARIANT == LMAZE_VARIANT_V4 || V5;   // "has a visit map"
    constexpr int C = V1 ? 4 : (V4 ? 7 : 5);
    // reset placement: row reads in flight per pass (mask_counts).  The two-level variants sit at the 128-VGPR step
    // (4 waves per SIMD) and any unrolling there costs a wave; v2/v4 have the room
    constexpr int PLACE_U = V5 ? 1 : 4;
    constexpr int PERENV = C * W25;  // floats of observation per env
    const int G = GT ? GT : a.p.grid, CELLS = G * G, L = V1 ? 1 : a.p.n_layouts;

    // LDS: per-env plane masks and window centres, the two 5x5 samples of the visit map (v4-v6), one
    // 64-bit row mask per layout row for each static plane, and the layout characters for the transition
    extern __shared__ int4 lds4[];
    // the 0/1 planes as bit strings, bit f = float f of the workgroup's contiguous output range (the float visit
    // planes of v4-v6 are zero bits there and come from vwin): a 16-byte store is one nibble of the string
    uint32_t* obits = reinterpret_cast<uint32_t*>(lds4);                   // [EPB*PERENV bits]  obs
    uint32_t* lbits = obits + EPB * 8;                                     // [EPB*100 bits]     obs_local (v5/v6)
    int16_t* cen = reinterpret_cast<int16_t*>(lbits + EPB * 4);            // [EPB][4]  cx, cy, px, py
    int32_t* flags = reinterpret_cast<int32_t*>(cen + EPB * 4);            // [EPB]     bit0 skip, bit1 visit update, bit2 fresh episode, bit3 not stepped
    int16_t* rcen = reinterpret_cast<int16_t*>(flags + EPB);               // [EPB][2]  ball a fused reset placed (visit map re-init)
    float* vwin = reinterpret_cast<float*>(rcen + EPB * 2);                // [EPB][2][25] visit-map samples (v4-v6)
    int32_t* clk = reinterpret_cast<int32_t*>(vwin + (V4 ? EPB * 2 * W25 : 0));   // [EPB] visit clock on entry (v4-v6)
    int32_t* dlist = clk + (V4 ? EPB : 0);                                 // [EPB] envs whose whole map is rewritten this call
    uint64_t* rowfree = reinterpret_cast<uint64_t*>(dlist + (V4 ? EPB : 0));   // [L*G] free = B|S|X
    uint64_t* rowgoal = rowfree + L * G;                                   // [L*G] interior, not 'W', not 'S' (v2:279)
    uint64_t* rowball = rowgoal + L * G;                                   // [L*G] interior, not 'W', not 'X' (v2:292)
    uint64_t* rowwall = rowball + L * G;                                   // [G] v1: 'W'
    uint64_t* rowx = rowwall + G;                                          // [G] v1: 'X'
    uint8_t* lays = reinterpret_cast<uint8_t*>(rowx + G);                  // [L*CELLS]
#if LMAZE_POL == 1
    uint8_t* ptab = lays + ((L * CELLS + 15) & ~15);                       // [L*CELLS] the policy table, when it is staged
    const FovealPol pol = ro.pol;
    const bool pstage = pol.in_lds != 0;
#elif LMAZE_POL == 2
    // [L*CELLS] rows of thresholds, when the table is staged: on the next 16-byte boundary of the allocation (the row masks
    // leave the characters on a multiple of 8 only), read with 128-bit LDS reads
    constexpr int SROW = V1 ? 4 : 24;                                      // words per key
    uint32_t* stab = reinterpret_cast<uint32_t*>(lds4) + ((((lays - reinterpret_cast<uint8_t*>(lds4)) + L * CELLS + 15) & ~15) >> 2);
    const FovealSmp smp = ro.smp;
    const bool pstage = smp.in_lds != 0;
#elif LMAZE_POL == 3
    // the controller table behind the characters and the planner table behind it, each only when it is staged
    const FovealHier hier = ro.hier;
    const int cbytes = hier_controller_bytes(hier.controller_key, L, G), pbytes = L * CELLS;
    const bool cstage = (hier.in_lds & kHierControllerStaged) != 0, pstage = (hier.in_lds & kHierPlannerStaged) != 0;
    uint8_t* ctab = lays + ((L * CELLS + 15) & ~15);
    uint8_t* ptab = ctab + (cstage ? (cbytes + 15) & ~15 : 0);
#elif LMAZE_POL == 4
    // the controller's rows on the next 16-byte boundary of the allocation behind the characters (POL 2's place) and the
    // planner's behind them, each only when it is staged; both sizes are multiples of 16
    const FovealHierSmp hsmp = ro.hsmp;
    const bool cstage = (hsmp.in_lds & kHierControllerStaged) != 0, pstage = (hsmp.in_lds & kHierPlannerStaged) != 0;
    const int ckeys = lmaze_hier_sample_controller_keys(hsmp.controller_key, L, G);
    uint32_t* ctab = reinterpret_cast<uint32_t*>(lds4) + ((((lays - reinterpret_cast<uint8_t*>(lds4)) + L * CELLS + 15) & ~15) >> 2);
    uint32_t* ptab = ctab + (cstage ? ckeys * LMAZE_HIER_SAMPLE_CROW : 0);
#endif
    static_assert(PERENV <= 8 * 32 - 32 && 4 * W25 <= 4 * 32 - 4, "bit strings fit the 32 B / 16 B per env reserved for them");
    __shared__ int any_skip, ndense;

    const int tid = threadIdx.x;
    // A workgroup takes chunks of EPB envs grid-stride (chunk = blockIdx.x, + gridDim.x, ...; one chunk each unless the
    // launcher asked for more): the set-up below -- row masks of all L layouts -- is paid once per workgroup while the
    // private range it streams at any moment stays one small chunk (lmaze_step.hip step_shared_kernel does the same)
    const int64_t nchunks = (a.n + EPB - 1) / EPB;
    int64_t chunk = blockIdx.x;
    int64_t blockbase = chunk * EPB;
    int nb = (int)min((int64_t)EPB, a.n - blockbase);
    if (tid == 0) { any_skip = 0; ndense = 0; }
    for (int i = tid; i < EPB * 12; i += LMAZE_BLOCK) obits[i] = 0u;       // obits and lbits
    if (V4) for (int i = tid; i < EPB * 2 * W25; i += LMAZE_BLOCK) vwin[i] = 0.0f;   // window cells outside the array read 0
    // the reset epoch, read in front of every store (one uniform scalar load; lmaze_step.hip step_shared_kernel)
    const uint64_t epoch = launch_epoch(a.epoch, a.epoch_in);
    if (MODE == FM_STEP && AR) pass_epoch_on(a.epoch_in, a.epoch_out);
    // large batches: the first 256 workgroups touch every 64-byte line of this step's action array at kernel
    // start, one burst of reads, so that the per-workgroup loads later in the launch hit the memory-side cache
    // instead of turning the saturated write stream around (lmaze_step.hip, step_shared_kernel)
    int warmed = 0;
    if (MODE == FM_STEP && !ROLL && a.nt) {
        warmed = warm_lines(a.action, a.n * 4, 256);
        // v1, v2: the per-env state as well (v2 -3 %).  v4 since its visit map is window-only (round 3: 334-338 us against
        // 341-377 without, three interleaved passes); v5/v6: no gain (418-443 against 425-465) -- experiment switch only
        if (!V5 || LMAZE_WARM_V4(a)) {
            warmed += warm_lines(a.b.ball_xy, a.n * 8, 256) + warm_lines(a.b.step_count, a.n * 4, 256);
            if (V1) warmed += warm_lines(a.b.fgoal_xy, a.n * 8, 256) + warm_lines(a.b.foveal_step_count, a.n * 4, 256);
            else warmed += warm_lines(a.b.goal_xy, a.n * 8, 256) + warm_lines(a.b.layout_id, a.n * 4, 256);
            if (V4) warmed += warm_lines(a.b.visit_clock, a.n * 4, 256);
            if (V5) warmed += warm_lines(a.b.fgoal_xy, a.n * 8, 256) + warm_lines(a.b.foveal_step_count, a.n * 4, 256) +
                              warm_lines(a.b.fovea_xy, a.n * 16, 256) + warm_lines(a.b.ball1_xy, a.n * 8, 256) +
                              warm_lines(a.b.last_xy, a.n * 8, 256) + warm_lines(a.b.foveal_goal, a.n * 4, 256) +
                              warm_lines(a.goal2, a.n * 4, 256);
        }
    }
    if (LMAZE_XP(a, 1)) {
        // experiment: no set-up
    } else if (GT != 0) {
        // Row masks by ballot, straight from global memory: a wave-iteration covers RPW whole layout rows (their
        // characters are RPW*G contiguous bytes, one per lane), four ballots give the rows' masks, and every load of
        // the workgroup -- these and the copy of the characters the transition looks cells up in -- is in flight
        // before the first is used.  One barrier.  (Round 1 copied the characters to LDS byte by byte, barrier, then
        // 90 lanes walked 18 LDS bytes each, twice: 58 of the 520 us of a v5 launch.)
        constexpr int GG = GT ? GT : 1, RPW = 64 / GG, UNR = 8;
        const int wave = tid >> 6, lane = tid & 63, rows = L * G;
        const int rsub = lane / GG, y = lane - rsub * GG;
        const bool dwords = ((reinterpret_cast<uintptr_t>(a.layouts) | (uintptr_t)(L * CELLS)) & 3) == 0;
        uint32_t cw[2] = {0u, 0u};
        if (dwords) {
#pragma unroll
            for (int j = 0; j < 2; ++j)
                if (tid + j * LMAZE_BLOCK < (L * CELLS) >> 2) cw[j] = reinterpret_cast<const uint32_t*>(a.layouts)[tid + j * LMAZE_BLOCK];
        }
#if LMAZE_POL == 1
        // the table is as large as the characters and indexed like them; its dwords are requested with theirs
        const bool pdwords = pstage && ((reinterpret_cast<uintptr_t>(pol.table) | (uintptr_t)(L * CELLS)) & 3) == 0;
        uint32_t pw[2] = {0u, 0u};
        if (pdwords) {
#pragma unroll
            for (int j = 0; j < 2; ++j)
                if (tid + j * LMAZE_BLOCK < (L * CELLS) >> 2) pw[j] = reinterpret_cast<const uint32_t*>(pol.table)[tid + j * LMAZE_BLOCK];
        }
#elif LMAZE_POL == 3
        // the staged tables' dwords are requested with the characters'
        const bool cdwords = cstage && ((reinterpret_cast<uintptr_t>(hier.controller) | (uintptr_t)cbytes) & 3) == 0;
        const bool pdwords = pstage && ((reinterpret_cast<uintptr_t>(hier.planner) | (uintptr_t)pbytes) & 3) == 0;
        uint32_t hcw[2], hpw[2];
        hier_request(hier.controller, cbytes, cdwords, tid, hcw);
        hier_request(hier.planner, pbytes, pdwords, tid, hpw);
#endif
        for (int r00 = 0; r00 < rows; r00 += UNR * 4 * RPW) {
            uint8_t cc[UNR];
#pragma unroll
            for (int u = 0; u < UNR; ++u) {
                const int row = r00 + (u * 4 + wave) * RPW + rsub;
                cc[u] = (rsub < RPW && row < rows) ? a.layouts[(size_t)row * G + y] : (uint8_t)0;
            }
#pragma unroll
            for (int u = 0; u < UNR; ++u) {
                const int row = r00 + (u * 4 + wave) * RPW + rsub;
                const bool in = rsub < RPW && row < rows;
                const uint8_t c = cc[u];
                const unsigned long long bf = __ballot(in && (c == 'B' || c == 'S' || c == 'X'));   // v1:78, v2:94
                const unsigned long long bw = __ballot(in && c == 'W');                              // v1:70
                const unsigned long long bx = __ballot(in && c == 'X');                              // v1:74
                const unsigned long long bs = __ballot(in && c == 'S');
                if (in && y == 0) {
                    const int sh = rsub * GG;
                    const uint64_t keep = GG == 64 ? ~0ull : ((1ull << GG) - 1ull);
                    const uint64_t fr = (bf >> sh) & keep, wl = (bw >> sh) & keep, xx = (bx >> sh) & keep, ss = (bs >> sh) & keep;
                    rowfree[row] = fr;
                    if (V1) { rowwall[row] = wl; rowx[row] = xx; }
                    if (!V1 && (MODE == FM_RESET || (MODE == FM_STEP && AR))) {
                        const int x = row % G;
                        const uint64_t interior = (x >= 1 && x <= G - 2) ? (((1ull << (G - 2)) - 1ull) << 1) : 0ull;
                        rowgoal[row] = fr & ~ss & interior;      // B or X
                        rowball[row] = fr & ~xx & interior;      // B or S
                    }
                }
            }
        }
        if (dwords) {
#pragma unroll
            for (int j = 0; j < 2; ++j)
                if (tid + j * LMAZE_BLOCK < (L * CELLS) >> 2) reinterpret_cast<uint32_t*>(lays)[tid + j * LMAZE_BLOCK] = cw[j];
            for (int i = tid + 2 * LMAZE_BLOCK; i < (L * CELLS) >> 2; i += LMAZE_BLOCK)     // more than 2 KiB of layouts
                reinterpret_cast<uint32_t*>(lays)[i] = reinterpret_cast<const uint32_t*>(a.layouts)[i];
        } else {
            for (int i = tid; i < L * CELLS; i += LMAZE_BLOCK) lays[i] = a.layouts[i];
        }
#if LMAZE_POL == 1
        if (pdwords) {
#pragma unroll
            for (int j = 0; j < 2; ++j)
                if (tid + j * LMAZE_BLOCK < (L * CELLS) >> 2) reinterpret_cast<uint32_t*>(ptab)[tid + j * LMAZE_BLOCK] = pw[j];
            for (int i = tid + 2 * LMAZE_BLOCK; i < (L * CELLS) >> 2; i += LMAZE_BLOCK)     // more than 2 KiB of table
                reinterpret_cast<uint32_t*>(ptab)[i] = reinterpret_cast<const uint32_t*>(pol.table)[i];
        } else if (pstage) {
            for (int i = tid; i < L * CELLS; i += LMAZE_BLOCK) ptab[i] = pol.table[i];
        }
#elif LMAZE_POL == 2
        if (pstage) stage_thresholds(stab, smp.table, L * CELLS * (SROW / 4), tid);
#elif LMAZE_POL == 3
        if (cstage) hier_stage(ctab, hier.controller, cbytes, cdwords, tid, hcw);
        if (pstage) hier_stage(ptab, hier.planner, pbytes, pdwords, tid, hpw);
#elif LMAZE_POL == 4
        if (cstage) stage_thresholds(ctab, hsmp.controller, ckeys * (LMAZE_HIER_SAMPLE_CROW / 4), tid);
        if (pstage) stage_thresholds(ptab, hsmp.planner, L * CELLS * (LMAZE_HIER_SAMPLE_PROW / 4), tid);
#endif
    } else {
    for (int i = tid; i < L * CELLS; i += LMAZE_BLOCK) lays[i] = a.layouts[i];
#if LMAZE_POL == 1
    if (pstage) for (int i = tid; i < L * CELLS; i += LMAZE_BLOCK) ptab[i] = pol.table[i];
#elif LMAZE_POL == 2
    if (pstage) stage_thresholds(stab, smp.table, L * CELLS * (SROW / 4), tid);
#elif LMAZE_POL == 3
    if (cstage) for (int i = tid; i < cbytes; i += LMAZE_BLOCK) ctab[i] = hier.controller[i];
    if (pstage) for (int i = tid; i < pbytes; i += LMAZE_BLOCK) ptab[i] = hier.planner[i];
#elif LMAZE_POL == 4
    if (cstage) stage_thresholds(ctab, hsmp.controller, ckeys * (LMAZE_HIER_SAMPLE_CROW / 4), tid);
    if (pstage) stage_thresholds(ptab, hsmp.planner, L * CELLS * (LMAZE_HIER_SAMPLE_PROW / 4), tid);
#endif
    __syncthreads();
    for (int i = tid; i < L * G; i += LMAZE_BLOCK) {
        uint64_t fr = 0, wl = 0, xx = 0;
        for (int y = 0; y < G; ++y) {
            const uint8_t c = lays[i * G + y];
            fr |= (uint64_t)(c == 'B' || c == 'S' || c == 'X') << y;       // v1:78, v2:94
            wl |= (uint64_t)(c == 'W') << y;                                // v1:70
            xx |= (uint64_t)(c == 'X') << y;                                // v1:74
        }
        rowfree[i] = fr;
        if (V1) { rowwall[i] = wl; rowx[i] = xx; }
        if (!V1 && (MODE == FM_RESET || (MODE == FM_STEP && AR))) {
            uint64_t ss = 0;
            for (int y = 0; y < G; ++y) ss |= (uint64_t)(lays[i * G + y] == 'S') << y;
            const int x = i % G;
            const uint64_t interior = (x >= 1 && x <= G - 2) ? (((1ull << (G - 2)) - 1ull) << 1) : 0ull;
            rowgoal[i] = fr & ~ss & interior;      // B or X
            rowball[i] = fr & ~xx & interior;      // B or S
        }
    }
    }
    __syncthreads();

    int t = 0;                                                             // rollout: step of the current chunk
#define ROLL_ROW(e) (ROLL ? (int64_t)t * a.n + (e) : (e))
#define ROLL_EP (ROLL ? epoch + (uint64_t)t : epoch)
  for (;;) {
    // ---------------- phase 1: one lane per env ----------------
    for (int le = tid; le < (LMAZE_XP(a, 8) ? 0 : nb); le += LMAZE_BLOCK) {
        const int64_t e = blockbase + le;
        EnvRec r;
        r.skip = 0; r.flat = -1; r.action = -1; r.lid = 0; r.gx = r.gy = -9;
        r.b0x = r.b0y = r.b1x = r.b1y = r.f1x = r.f1y = 0; r.upd = 0; r.pad = 0;
        bool fresh = false, nostep = false;   // fused reset: new episode this call / its step was refused
        bool last_is_cur = true;              // v5/v6: the window shown as "previous" from now on is this call's current one
        int rx = 0, ry = 0;                   // ball the fused reset placed
        float row_r = -0.0f, row_fr = -0.0f;  // rollout: the env's reward / done after this step (trajectory rows)
        int row_d = 0, row_fd = 0;
        int bx = a.b.ball_xy[2 * e], by = a.b.ball_xy[2 * e + 1];
        // every per-env input of a step is requested HERE, before anything is branched on: a load that sits behind a branch
        // on another loaded value (the done flag of the fused reset, localDone of the two-level step) is a second global
        // round trip in series -- v4's fused reset cost +58...95 us per launch that way (round 3, tools/_ar_study)
        // rollout: step t takes row t of the actions and planner goals (ROLL_ROW), and its resets draw with epoch + t (ROLL_EP)
#if LMAZE_POL
        const int act_in = 0;                 // no action tensor: the table and the draw, after the fused reset
#else
        const int act_in = (MODE == FM_STEP) ? a.action[ROLL_ROW(e)] : 0;
#endif
        const int sc_ld = (MODE == FM_STEP) ? a.b.step_count[e] : 0;
        const int done_in = (MODE == FM_STEP && AR) ? a.b.done[e] : 0;
#if LMAZE_POL != 3 && LMAZE_POL != 4
        const int goal2_in = (MODE == FM_STEP && AR && V5) ? a.goal2[ROLL_ROW(e)] : 0;
#endif
        const int vword = (V4 && !(V5 && MODE == FM_PLANNER)) ? a.b.visit_clock[e] : 0;
        const int vclock = vword & 0xff;
#if LMAZE_POL == 2
        // the sampling draw, on every env-step: one word of it is live across the fused reset.  It depends on nothing loaded,
        // so it stands in front of the placement chain and runs under the loads above.
        const uint32_t prx = policy_draw(a.seed, ROLL_EP, a.env_base + e).x;
#elif LMAZE_POL == 3
        // one draw for both levels, only when either explores (uniform over the launch): in front of the placement chain
        uint4 pr = make_uint4(0u, 0u, 0u, 0u);
        if ((hier.epsilon | hier.planner_epsilon) != 0u) pr = policy_draw(a.seed, ROLL_EP, a.env_base + e);
#elif LMAZE_POL == 4
        // one draw for both levels, on every env-step: two words of it are live across the fused reset.  In front of the
        // placement chain, under the loads above.
        const uint4 pr4 = policy_draw(a.seed, ROLL_EP, a.env_base + e);
        const uint32_t prx = pr4.x, prz = pr4.z;
#elif LMAZE_POL
        // the exploration draw, only when there is exploration (uniform over the launch).  It depends on nothing loaded, so
        // it stands in front of the fused reset's placement chain and runs under the loads above.
        uint4 pr = make_uint4(0u, 0u, 0u, 0u);
        if (pol.epsilon != 0u) pr = policy_draw(a.seed, ROLL_EP, a.env_base + e);
#endif
        r.px = (int16_t)bx; r.py = (int16_t)by;
        if (MODE != FM_STEP && a.mask && !a.mask[e]) r.skip = 1;
        if (V1) {
            int fgx = a.b.fgoal_xy[2 * e], fgy = a.b.fgoal_xy[2 * e + 1];
            r.action = 1;  // local view unless this is a reset
            if (MODE == FM_STEP) {
                int sc_in = sc_ld;
                if (AR && done_in) {                         // fused reset(): v1:82-93
                    for (int c = 0; c < CELLS; ++c)
                        if (lays[c] == 'S') { bx = c / G; by = c % G; break; }
                    sc_in = 0;
                }
#if LMAZE_POL == 2
                const int act = foveal_smp_action<true>(smp, pstage, stab, 0, bx, by, G, 1, prx, ROLL_ROW(e));   // the key is the placed ball's
#elif LMAZE_POL == 1
                const int act = foveal_pol_action(pol, pstage, ptab, 0, bx, by, G, 1, 4, pr, ROLL_ROW(e));   // the key is the placed ball's
#else
                const int act = act_in;
#endif
                const int sc = sc_in + 1;                              // v1:117
                const int fsc = a.b.foveal_step_count[e] + 1;          // v1:118
                float fr = -0.0f, rw = -0.0f;                          // v1:120-121
                bool local_done = false;                               // v1:123
                int ox, oy;
                decode_action(act, ox, oy);                            // v1:125-133
                const int tx = clampi(bx + ox, 0, G - 1), ty = clampi(by + oy, 0, G - 1);
                const uint8_t c = lays[tx * G + ty];
                if (c == 'W') {                                        // v1:135-138
                    rw = a.p.reward_wall; fr = a.p.reward_wall;
                } else if (c == 'B') {                                 // v1:140-163
                    bx = tx; by = ty;
                    rw = a.p.reward_move; fr = a.p.reward_move;
                    if (bx < fgx - 1 || bx > fgx + 2 || by < fgy - 1 || by > fgy + 2) {
                        local_done = true; fr = a.p.reward_wall;
                    } else if (by == fgy && bx == fgx) {
                        local_done = true; fr = a.p.reward_goal;
                    }
                } else if (c == 'X') {                                 // v1:165-183
                    bx = tx; by = ty;
                    rw = a.p.reward_goal;
                    if (by == fgy && bx == fgx) { local_done = true; fr = a.p.reward_goal; }
                    else fr = a.p.reward_move;
                }
                const bool done = (rw == a.p.reward_goal) || (sc == a.p.step_limit);                         // v1:294-304
                const bool fdone = local_done || fr == a.p.reward_goal || fsc == a.p.foveal_step_limit || done;  // v1:308-324
                a.b.ball_xy[2 * e] = bx; a.b.ball_xy[2 * e + 1] = by;
                a.b.step_count[e] = sc; a.b.foveal_step_count[e] = fsc;
                a.b.reward[e] = rw; a.b.foveal_reward[e] = fr;
                a.b.done[e] = done ? 1 : 0; a.b.foveal_done[e] = fdone ? 1 : 0;
                row_r = rw; row_fr = fr; row_d = done; row_fd = fdone;
            } else if (MODE == FM_RESET && !r.skip) {
                if (a.place) {                                         // v1:82-84: ball = first 'S'
                    for (int c = 0; c < CELLS; ++c)
                        if (lays[c] == 'S') { bx = c / G; by = c % G; break; }
                    a.b.ball_xy[2 * e] = bx; a.b.ball_xy[2 * e + 1] = by;
                }
                a.b.reward[e] = -0.0f; a.b.foveal_reward[e] = -0.0f;   // v1:90-91
                a.b.step_count[e] = 0;                                 // v1:93 (fovealStepCount kept, v1:94)
                a.b.done[e] = 0; a.b.foveal_done[e] = 0;
                r.action = 0;                                          // v1:100 getGlobalView
            } else if (MODE == FM_SETGOAL && !r.skip) {                // v1:104-110
                fgx = bx + a.action[2 * e] - 2;
                fgy = by + a.action[2 * e + 1] - 2;
                a.b.fgoal_xy[2 * e] = fgx; a.b.fgoal_xy[2 * e + 1] = fgy;
                a.b.foveal_step_count[e] = 0;
            }
            int flat = fgx * G + fgy;                                  // v1:244-245, numpy negative-index wrap
            if (flat < 0) flat += CELLS;
            r.flat = (flat >= 0 && flat < CELLS) ? flat : -1;
        } else if (V5) {
            int lid = clampi(a.b.layout_id[e], 0, L - 1);
            int gx = a.b.goal_xy[2 * e], gy = a.b.goal_xy[2 * e + 1];
            int fg = a.b.foveal_goal[e];
            int f0x = a.b.fovea_xy[4 * e], f0y = a.b.fovea_xy[4 * e + 1];
            int f1x = a.b.fovea_xy[4 * e + 2], f1y = a.b.fovea_xy[4 * e + 3];
            int b1x = a.b.ball1_xy[2 * e], b1y = a.b.ball1_xy[2 * e + 1];
            int lx = a.b.last_xy[2 * e], ly = a.b.last_xy[2 * e + 1];
            if (MODE == FM_STEP) {                                     // v5:187-292
#if LMAZE_POL == 3 || LMAZE_POL == 4
                int act = act_in;                                      // the controller's, once the planner has stepped
#else
                const int act = act_in;
#endif
                int fgx = a.b.fgoal_xy[2 * e], fgy = a.b.fgoal_xy[2 * e + 1];
                int fsc = a.b.foveal_step_count[e];
                int sc_in = sc_ld;
                bool ld = a.b.foveal_done[e] != 0, gd = a.b.done[e] != 0;   // both persist across step() calls
                if (AR) {
                    // the two-level loop around step() (lmaze_v5_hier_step): reset() for an env that enters with
                    // globalDone, plannerStep(goal) for one that enters with localDone or was just reset
                    const bool plan = ld || gd;
                    bool planned = false;
                    if (gd) {                                          // reset(): v5:104-150, as FM_RESET below
                        const uint4 d = env_draw(a.seed, ROLL_EP, a.env_base + e);
                        lid = (int)__umulhi(d.z, (uint32_t)L);         // v5:105 setGrid first
                        int goal_cell, ball_cell;
                        place_goal_ball<PLACE_U>(rowgoal + lid * G, rowball + lid * G, G, d, goal_cell, ball_cell);
                        if (goal_cell >= 0) { gx = goal_cell / G; gy = goal_cell % G; }
                        if (ball_cell >= 0) { bx = ball_cell / G; by = ball_cell % G; }
                        a.b.layout_id[e] = lid;
                        a.b.goal_xy[2 * e] = gx; a.b.goal_xy[2 * e + 1] = gy;
                        fsc = 0; sc_in = 0; gd = false; ld = false;    // v5:109-112
                        fg = 12;                                       // v5:127-128
                        f0x = f1x = b1x = lx = fgx = bx; f0y = f1y = b1y = ly = fgy = by;   // v5:136-143
                        fresh = true;
                    }
                    if (plan) {                                        // plannerStep(goal): v5:158-182, as FM_PLANNER below
#if LMAZE_POL == 3
                        const int g = hier_plan_goal(hier, ptab, lid, bx, by, G, L, pr.z, pr.w, ROLL_ROW(e));   // the state after the reset
#elif LMAZE_POL == 4
                        const int g = hier_smp_goal(hsmp, ptab, lid, bx, by, G, L, prz, ROLL_ROW(e));   // the state after the reset; 0..24
#else
                        const int g = goal2_in;
#endif
                        if (g >= 0 && g < W25) {
                            fg = g;
                            sc_in = 0;                                 // v5:160
                            ld = false;                                // v5:162
                            fgx = bx + g / FOV - 2; fgy = by + g % FOV - 2;   // v5:172-173
                            if (fsc > 0) { f1x = f0x; f1y = f0y; }     // v5:175-177
                            fsc += 1;                                  // v5:179
                            planned = true;
                        }
                    }
#if LMAZE_POL == 3
                    else hier_no_goal(hier, ROLL_ROW(e));
#elif LMAZE_POL == 4
                    else hier_smp_no_goal(hsmp, ROLL_ROW(e));
#endif
                    if (fresh || planned) {
                        a.b.foveal_goal[e] = fg;
                        a.b.fgoal_xy[2 * e] = fgx; a.b.fgoal_xy[2 * e + 1] = fgy;
                        a.b.fovea_xy[4 * e + 2] = f1x; a.b.fovea_xy[4 * e + 3] = f1y;
                        a.b.foveal_step_count[e] = fsc;
                    }
                }
#if LMAZE_POL == 3
                act = hier_act(hier, ctab, lid, bx, by, fgx, fgy, G, L, pr.x, pr.y, ROLL_ROW(e));   // the state after the plannerStep
#elif LMAZE_POL == 4
                act = hier_smp_act(hsmp, ctab, lid, bx, by, fgx, fgy, G, L, prx, ROLL_ROW(e));   // the state after the plannerStep
#endif
                const uint8_t* lay = lays + lid * CELLS;
                b1x = bx; b1y = by;                                    // v5:193-194
                float lr = -0.0f, gr;                                  // v5:196
                const int sc = sc_in + 1;                              // v5:197
                const int dx = (act == 0) - (act == 1), dy = (act == 2) - (act == 3);   // v5:205-217
                const int nx = bx + dx, ny = by + dy;
                const bool nin = nx >= 0 && ny >= 0 && nx < G && ny < G;
                const uint8_t c = nin ? lay[nx * G + ny] : (uint8_t)'W';
                if (c == 'W') {                                        // v5:232-233
                    lr = a.p.reward_wall;
                } else if (nx == fgx && ny == fgy) {                   // v5:235-239
                    lr = a.p.reward_goal; bx = nx; by = ny; ld = true;
                } else if (c == 'B' || c == 'S' || c == 'X') {         // v5:241-248
                    if (nx < f1x - 3 || nx > f1x + 2 || ny < f1y - 3 || ny > f1y + 2) ld = true;
                    lr = a.p.reward_move; bx = nx; by = ny;
                }
                if (nx == gx && ny == gy) { gr = a.p.reward_goal; gd = true; }   // v5:254-262
                else if (nx == fgx && ny == fgy) gr = a.p.reward_move;
                else gr = a.p.reward_wall;
                f0x = bx; f0y = by;                                    // v5:264-265
                if (sc >= a.p.step_limit) ld = true;                   // v5:267
                if (fsc >= a.p.foveal_step_limit) { gd = true; ld = true; }   // v5:269-271
                if (fsc == 0) { lx = f0x; ly = f0y; }                  // v5:322-323
                r.px = (int16_t)lx; r.py = (int16_t)ly;                // window the foveal obs shows as "previous"
                r.upd = ld ? 1 : 0;                                    // v5:313-318
                if (ld) { lx = f0x; ly = f0y; }                        // v5:344-346 (after the render)
                last_is_cur = lx == f0x && ly == f0y;
                a.b.ball_xy[2 * e] = bx; a.b.ball_xy[2 * e + 1] = by;
                a.b.ball1_xy[2 * e] = b1x; a.b.ball1_xy[2 * e + 1] = b1y;
                a.b.fovea_xy[4 * e] = f0x; a.b.fovea_xy[4 * e + 1] = f0y;
                a.b.last_xy[2 * e] = lx; a.b.last_xy[2 * e + 1] = ly;
                a.b.step_count[e] = sc;
                a.b.reward[e] = gr; a.b.foveal_reward[e] = lr;
                a.b.done[e] = gd ? 1 : 0; a.b.foveal_done[e] = ld ? 1 : 0;
                row_r = gr; row_fr = lr; row_d = gd; row_fd = ld;
            } else if (MODE == FM_PLANNER && !r.skip) {                // v5:158-182
                const int g = a.action[e];
                if (g < 0 || g >= W25) {
                    r.skip = 1;                                        // the reference raises half-way (v5:169)
                } else {
                    fg = g;
                    a.b.step_count[e] = 0;                             // v5:160
                    a.b.reward[e] = -0.0f;                             // v5:161
                    a.b.foveal_done[e] = 0;                            // v5:162
                    a.b.foveal_goal[e] = g;
                    a.b.fgoal_xy[2 * e] = bx + g / FOV - 2;            // v5:172-173
                    a.b.fgoal_xy[2 * e + 1] = by + g % FOV - 2;
                    const int fsc = a.b.foveal_step_count[e];
                    if (fsc > 0) {                                     // v5:175-177
                        f1x = f0x; f1y = f0y;
                        a.b.fovea_xy[4 * e + 2] = f1x; a.b.fovea_xy[4 * e + 3] = f1y;
                    }
                    a.b.foveal_step_count[e] = fsc + 1;                // v5:179
                }
            } else if (MODE == FM_RESET && !r.skip) {                  // v5:104-150
                if (a.place) {
                    const uint4 d = env_draw(a.seed, a.epoch, a.env_base + e);
                    lid = (int)__umulhi(d.z, (uint32_t)L);             // v5:105 setGrid first
                    a.b.layout_id[e] = lid;
                    int goal_cell, ball_cell;
                    place_goal_ball<PLACE_U>(rowgoal + lid * G, rowball + lid * G, G, d, goal_cell, ball_cell);
                    if (goal_cell >= 0) {
                        gx = goal_cell / G; gy = goal_cell % G;
                        a.b.goal_xy[2 * e] = gx; a.b.goal_xy[2 * e + 1] = gy;
                    }
                    if (ball_cell >= 0) {
                        bx = ball_cell / G; by = ball_cell % G;
                        a.b.ball_xy[2 * e] = bx; a.b.ball_xy[2 * e + 1] = by;
                    }
                }
                a.b.foveal_reward[e] = -0.0f; a.b.reward[e] = -0.0f;   // v5:107-108
                a.b.foveal_step_count[e] = 0; a.b.step_count[e] = 0;   // v5:109-110
                a.b.done[e] = 0; a.b.foveal_done[e] = 0;               // v5:111-112
                fg = 12;                                               // v5:127-128
                a.b.foveal_goal[e] = fg;
                f0x = f1x = b1x = lx = bx; f0y = f1y = b1y = ly = by;  // v5:136-143
                a.b.fovea_xy[4 * e] = bx; a.b.fovea_xy[4 * e + 1] = by;
                a.b.fovea_xy[4 * e + 2] = bx; a.b.fovea_xy[4 * e + 3] = by;
                a.b.fgoal_xy[2 * e] = bx; a.b.fgoal_xy[2 * e + 1] = by;
                a.b.ball1_xy[2 * e] = bx; a.b.ball1_xy[2 * e + 1] = by;
                a.b.last_xy[2 * e] = bx; a.b.last_xy[2 * e + 1] = by;
                r.px = (int16_t)bx; r.py = (int16_t)by;
            }
            r.lid = (int16_t)lid;
            r.gx = (int16_t)gx; r.gy = (int16_t)gy;
            r.action = (int16_t)fg;
            r.b0x = (int16_t)bx; r.b0y = (int16_t)by; r.b1x = (int16_t)b1x; r.b1y = (int16_t)b1y;
            r.f1x = (int16_t)f1x; r.f1y = (int16_t)f1y;
            bx = f0x; by = f0y;                                        // the window centre is fovea_0
        } else {
            int lid = a.b.layout_id[e];
            int gx = a.b.goal_xy[2 * e], gy = a.b.goal_xy[2 * e + 1];
            int sc_in = 0;
            const bool fused = MODE == FM_STEP && AR && done_in != 0;
            if ((MODE == FM_RESET && !r.skip) || fused) {              // reset(): v2:80-123, v4:95-163
                if (a.place || fused) {
                    const uint4 d = env_draw(a.seed, ROLL_EP, a.env_base + e);
                    const int lid_new = (int)__umulhi(d.z, (uint32_t)L);
                    if (V4) lid = lid_new;                             // v4:97 setGrid first
                    lid = clampi(lid, 0, L - 1);
                    int goal_cell, ball_cell;
                    place_goal_ball<PLACE_U>(rowgoal + lid * G, rowball + lid * G, G, d, goal_cell, ball_cell);
                    if (goal_cell >= 0) {
                        gx = goal_cell / G; gy = goal_cell % G;
                        a.b.goal_xy[2 * e] = gx; a.b.goal_xy[2 * e + 1] = gy;
                    }
                    if (ball_cell >= 0) {
                        bx = ball_cell / G; by = ball_cell % G;
                        a.b.ball_xy[2 * e] = bx; a.b.ball_xy[2 * e + 1] = by;
                    }
                    lid = lid_new;                                     // v2:92 setGrid last
                    a.b.layout_id[e] = lid;
                }
                a.b.reward[e] = -0.0f;                                 // v2:84
                a.b.step_count[e] = 0;                                 // v2:86
                a.b.done[e] = 0;
                r.px = (int16_t)bx; r.py = (int16_t)by;                // v2:109: previous = current
                fresh = true;
                rx = bx; ry = by;
            } else if (MODE == FM_STEP) {
                sc_in = sc_ld;
            }
            if (MODE == FM_STEP) {
#if LMAZE_POL == 2
                const int act = foveal_smp_action<false>(smp, pstage, stab, lid, bx, by, G, L, prx, ROLL_ROW(e));   // the row the step uses
#elif LMAZE_POL == 1
                const int act = foveal_pol_action(pol, pstage, ptab, lid, bx, by, G, L, W25, pr, ROLL_ROW(e));   // the row the step uses
#else
                const int act = act_in;
#endif
                if (act < 0 || act >= W25) {
                    if (fresh) nostep = true;                          // reset, then the reference's step() raises
                    else r.skip = 1;                                   // the reference raises before touching anything
                    if (ROLL && !fresh) { row_r = a.b.reward[e]; row_d = a.b.done[e]; }   // rows: as the step left them
                } else {
                    lid = clampi(lid, 0, L - 1);
                    const uint8_t* lay = lays + lid * CELLS;
                    float rw = -0.0f;                                  // v2:146
                    const int sc = sc_in + 1;                          // v2:147
                    const int fx = bx + act / FOV - 2, fy = by + act % FOV - 2;   // v2:151-152
                    if (fx < G - 2 && fx > 1 && fy < G - 2 && fy > 1) {           // v2:157-159
                        bx = fx; by = fy;
                    } else {                                           // v2:160-169
                        if (fx >= G - 2) bx = G - 3;
                        if (fx <= 1) bx = 2;
                        if (fy >= G - 2) by = G - 3;
                        if (fy <= 1) by = 2;
                    }
                    const bool fin = fx >= 0 && fy >= 0 && fx < G && fy < G;
                    const uint8_t c = fin ? lay[fx * G + fy] : (uint8_t)'W';
                    if (fx == gx && fy == gy) rw = a.p.reward_goal;    // v2:175-180
                    else if (c == 'W') rw = a.p.reward_wall;
                    else if (c == 'B' || c == 'S') rw = a.p.reward_move;
                    a.b.ball_xy[2 * e] = bx; a.b.ball_xy[2 * e + 1] = by;
                    a.b.step_count[e] = sc;
                    a.b.reward[e] = rw;
                    a.b.done[e] = (rw == a.p.reward_goal || sc > a.p.step_limit) ? 1 : 0;   // v2:222
                    r.action = (int16_t)act;
                    row_r = rw; row_d = rw == a.p.reward_goal || sc > a.p.step_limit;
                }
            }
            r.lid = (int16_t)clampi(lid, 0, L - 1);
            r.gx = (int16_t)gx; r.gy = (int16_t)gy;
        }
        r.cx = (int16_t)bx; r.cy = (int16_t)by;
        // the observation as 25-bit planes (the float visit planes are sampled in phase 3)
        uint32_t m[8];
        if (V1) {
            m[0] = 1u << 12;                                                               // ball, v1:216
            m[1] = window_bits(rowwall, G, r.cx, r.cy);
            m[2] = r.action ? (r.flat >= 0 ? onehot_bits(r.flat / G, r.flat % G, r.cx, r.cy) : 0u)   // v1:244-245
                            : window_bits(rowx, G, r.cx, r.cy);
            m[3] = window_bits(rowfree, G, r.cx, r.cy);
        } else {
            constexpr int PER = VARIANT == LMAZE_VARIANT_V2 ? 2 : 3;
            const uint64_t* rows = rowfree + r.lid * G;
            m[0] = window_bits(rows, G, r.cx, r.cy);                                       // v2:94
            m[1] = onehot_bits(r.gx, r.gy, r.cx, r.cy);                                    // v2:95
            m[PER] = (r.action >= 0 && r.action < W25) ? (1u << r.action) : 0u;            // v2:135-136, v5:166-169
            m[PER + 1] = window_bits(rows, G, r.px, r.py);
            m[PER + 2] = onehot_bits(r.gx, r.gy, r.px, r.py);
            if (V5) {                                                                      // v5:356-380
                uint32_t lm[4];
                lm[0] = m[0];
                const int i0 = wrap5(r.b0x - r.f1x + 2), j0 = wrap5(r.b0y - r.f1y + 2);
                const int i1 = wrap5(r.b1x - r.f1x + 2), j1 = wrap5(r.b1y - r.f1y + 2);
                lm[1] = (i0 >= 0 && j0 >= 0) ? (1u << (FOV * i0 + j0)) : 0u;
                lm[2] = (i1 >= 0 && j1 >= 0) ? (1u << (FOV * i1 + j1)) : 0u;
                lm[3] = m[PER];
                if (MODE != FM_RESET && !r.skip)
                    for (int ch = 0; ch < 4; ++ch) put_bits(lbits, le * (4 * W25) + ch * W25, lm[ch]);
            }
        }
        if (!r.skip) {
#pragma unroll
            for (int ch = 0; ch < C; ++ch)
                if (!(V4 && (ch == 2 || ch == 6))) put_bits(obits, le * PERENV + ch * W25, m[ch]);
        }
        cen[le * 4 + 0] = r.cx; cen[le * 4 + 1] = r.cy; cen[le * 4 + 2] = r.px; cen[le * 4 + 3] = r.py;
        int fl = (r.skip ? 1 : 0) | (r.upd ? 2 : 0) | (fresh ? 4 : 0) | (nostep ? 8 : 0);
        if (V4 && !(V5 && MODE == FM_PLANNER) && !r.skip) {
            // What this call does to the env's visit map, in clock terms (phase 2 carries it out on the cells):
            //   zero    reset(): the map restarts from zeros, clock 0 (v4:112, v5:130)
            //   renorm  the clock is about to leave the exponent range: rewrite the map in true values, clock VISIT_BIAS
            //   pre     fused reset of v4: the reset's own (0 + window) / 2 at the placed ball (v4:116-119)
            //   add     this call's (map + window) / 2 at the window centre: v4 every step and every reset
            //           (v4:211-214), v5/v6 only on localDone (v5:313-318) and never at reset (v5:130)
            const bool zero = MODE == FM_RESET || (MODE == FM_STEP && AR && fresh);
            const bool renorm = !zero && vclock >= VISIT_RENORM;
            const bool pre = !V5 && MODE == FM_STEP && AR && fresh;
            const bool add = !(V5 && MODE == FM_RESET) && !nostep && !(V5 && MODE == FM_STEP && !r.upd);
            // the "previous window" record behind the tiles: it must hold the window the NEXT call shows as previous, in
            // true values -- this call's current window (cw0: v4 always; v5/v6 when retStatelast moved, v5:322-346), or
            // the previous one as this call left it (cw1: the map or the episode changed under it)
            const bool cw0 = V5 && (MODE == FM_RESET || last_is_cur);
            const bool cw1 = V5 && !cw0 && (fresh || add);
            // v5/v6: does the env's record hold the window this call shows as "previous"?  (a freshly loaded state does not)
            const bool hit = V5 && !zero && (vword >> 8) == (visit_tag(r.px, r.py) >> 8);
            fl |= (zero ? 16 : 0) | (renorm ? 32 : 0) | (pre ? 64 : 0) | (add ? 128 : 0) | (cw0 ? 256 : 0) | (cw1 ? 512 : 0) | (hit ? 1024 : 0);
            int c1 = (zero ? 0 : (renorm ? VISIT_BIAS : vclock)) + (pre ? 1 : 0) + (add ? 1 : 0);
            // the record's tag: the centre it will hold after this call (cw0 / cw1), else as it was
            if (V5) c1 |= cw0 ? visit_tag(r.cx, r.cy) : (cw1 ? visit_tag(r.px, r.py) : (vword & ~0xff));
            if (c1 != vword) a.b.visit_clock[e] = c1;
            if (zero || renorm) dlist[atomicAdd(&ndense, 1)] = le;
        }
        if (V4) clk[le] = vclock;
        flags[le] = fl;
        rcen[le * 2] = (int16_t)rx; rcen[le * 2 + 1] = (int16_t)ry;
        if (r.skip) any_skip = 1;
        if (ROLL) {
            const int64_t o = (int64_t)t * a.n + e;                  // T*N passes 2^31 at 1M envs x 4096 steps
            if (ro.reward_t) ro.reward_t[o] = row_r;
            if (ro.done_t) ro.done_t[o] = (uint8_t)row_d;
            if (V1 || V5) {
                if (ro.freward_t) ro.freward_t[o] = row_fr;
                if (ro.fdone_t) ro.fdone_t[o] = (uint8_t)row_fd;
            }
        }
    }
    __syncthreads();
    const bool some_skipped = any_skip != 0;

    // ---------------- phase 2 (v4-v6): the visit maps, v4:116-119 / v4:211-214 / v5:313-318 ----------------
    // Clock-relative tiles (include/lmaze.h "The visit map"): the whole-plane halving already happened in phase 1 (the
    // env's clock moved); what is left is the 5x5 window.  The few envs whose whole map is rewritten (reset: zeros; clock at
    // VISIT_RENORM: true values) are streamed tile by tile; everybody else goes through the window pass below, one lane per
    // window row.  (Tried and dropped this round, LAB_NOTES.md R3.1 / R3.5: one lane per TILE row -- the bookkeeping made the
    // phase issue-bound --, whole tiles staged in LDS by LDS-DMA -- 640 B of LDS per env --, one wave instruction per env, and
    // a software-pipelined chunk loop that issues the next chunk's phase 1 and tile loads before this chunk's stores --
    // 45 registers of loads held across the store phase: 171-214 VGPRs, 2-3 waves per SIMD, 357 / 552 us against 296 / 422.)
    if (V4 && !(V5 && MODE == FM_PLANNER) && !LMAZE_XP(a, 32)) {
        const int TB = visit_tiles(G), TILES = TB * TB;
        uint32_t* vis = reinterpret_cast<uint32_t*>(a.b.visit) + (size_t)blockbase * TILES * (VT * VT);
        uint32_t* rec = reinterpret_cast<uint32_t*>(a.b.visit) + (size_t)a.n * TILES * (VT * VT) + (size_t)blockbase * VPC;
        // One tile row of an env whose WHOLE map is rewritten this call: zeros (reset) or true values (clock at
        // VISIT_RENORM) first, then the fused reset's own window at the placed ball (`pre`, v4:116-119), then `add`.
        auto tile_row_whole = [&](uint32_t (&s)[4], int x, int y0, int le, int fl) {
            const int E0 = clk[le];
            const bool zero = fl & 16, renorm = fl & 32, pre = fl & 64, add = fl & 128;
            const int cx = cen[le * 4], cy = cen[le * 4 + 1], px = cen[le * 4 + 2], py = cen[le * 4 + 3];
            const int E1 = zero ? 0 : (renorm ? VISIT_BIAS : E0);
            const int dx = x - cx + 2, ex = x - px + 2;
#pragma unroll 1
            for (int k = 0; k < 4; ++k) {
                const int y = y0 + k;
                const bool cell_ok = x < G && y < G;      // tiles are padded up to a multiple of 4: those cells stay 0
                uint32_t b = s[k];
                if (zero) b = 0u;
                else if (renorm) b = visit_true(b, E0);
                int E = E1;
                if (pre) {
                    const int qx = x - rcen[le * 2] + 2, qy = y - rcen[le * 2 + 1] + 2;
                    if (cell_ok && (unsigned)qx <= 4u && (unsigned)qy <= 4u) b = visit_add(b, E);
                    ++E;
                }
                const int dy = y - cy + 2, ey = y - py + 2;
                const bool in = cell_ok && (unsigned)dx <= 4u && (unsigned)dy <= 4u;
                if (add) {
                    if (in) b = visit_add(b, E);
                    ++E;
                }
                s[k] = b;
                if (in) vwin[le * 2 * W25 + dx * FOV + dy] = __uint_as_float(visit_true(b, E));
                if (cell_ok && (unsigned)ex <= 4u && (unsigned)ey <= 4u)
                    vwin[le * 2 * W25 + W25 + ex * FOV + ey] = __uint_as_float(visit_true(b, E));
            }
        };
        // ---- whole maps first: envs that were reset (zeros, nothing loaded) or whose clock reached VISIT_RENORM
        {
            const int nd = ndense, per = TILES * VT;
            for (int j = tid; j < nd * per; j += LMAZE_BLOCK) {
                const int d = j / per, r = j - d * per;
                const int le = dlist[d], fl = flags[le];
                const int tile = r >> 2, row = r & 3;
                const int tx = tile / TB, ty = tile - tx * TB;
                uint32_t* p = vis + (le * TILES + tile) * (VT * VT) + row * VT;
                uint32_t sv[4] = {0u, 0u, 0u, 0u};
                if (!(fl & 16)) {
                    const uint4 t4 = *reinterpret_cast<const uint4*>(p);
                    sv[0] = t4.x; sv[1] = t4.y; sv[2] = t4.z; sv[3] = t4.w;
                }
                tile_row_whole(sv, tx * VT + row, ty * VT, le, fl & 0xff);
                *reinterpret_cast<uint4*>(p) = make_uint4(sv[0], sv[1], sv[2], sv[3]);
            }
        }
        // ---- the windows: ONE LANE PER WINDOW ROW.  Item = (env, window 0: current / 1: "previous", row 0..4): the row's
        // five cells lie in two horizontally adjacent tiles, on one tile row each -- two 16-byte loads, eight words, the
        // five wanted ones start at word y0 & 3 --, or, v5/v6, in the env's "previous window" record (20 contiguous
        // bytes) when that window lies elsewhere.  Every load of the chunk is in flight before the first is used, and
        // nothing is stored before every lane has its loads (the barrier): a cell both windows show is loaded by two
        // lanes and each works out the same new value for it.  Cells of the current window take (v + 1) / 2 when the map
        // updates this call and the two 16-byte pieces go back re-encoded under the new clock (into lines the loads have
        // just brought into L2); the TRUE values both windows show -- the previous one sampled live from the updated
        // map, Appendix B-7 -- are left in vwin for phase 3.
        {
            // SUB envs at a time (one barrier each): the loads of a pass are held in registers, 9 per row
#if LMAZE_POL == 2
            // as the epsilon-greedy form below; the fused recording form at a generic grid has no registers for it either
            constexpr int WSUB = (REC && (!AR || GT == 0)) ? 32 : LMAZE_WIN_SUB;
            constexpr int IPE = 2 * FOV, SUB = EPB < WSUB ? EPB : WSUB, NIT = (SUB * IPE + LMAZE_BLOCK - 1) / LMAZE_BLOCK;
#elif LMAZE_POL == 1
            // the plain recording form of the closed loop has no registers for a third window row per lane
            constexpr int IPE = 2 * FOV, SUB = EPB < ((REC && !AR) ? 32 : LMAZE_WIN_SUB) ? EPB : ((REC && !AR) ? 32 : LMAZE_WIN_SUB);
            constexpr int NIT = (SUB * IPE + LMAZE_BLOCK - 1) / LMAZE_BLOCK;
#else
            constexpr int IPE = 2 * FOV, SUB = EPB < LMAZE_WIN_SUB ? EPB : LMAZE_WIN_SUB, NIT = (SUB * IPE + LMAZE_BLOCK - 1) / LMAZE_BLOCK;
#endif
          for (int sb = 0; sb < nb; sb += SUB) {
            const int items = LMAZE_XP(a, 256) ? 0 : min(SUB, nb - sb) * IPE;
            uint4 va[NIT], vb[NIT];
            int meta[NIT];    // -1 nothing; else global word offset of piece A (tiles) or of the row (record) | 1 << 28 record | 1 << 29 piece A outside | 1 << 30 piece B outside
#pragma unroll
            for (int u = 0; u < NIT; ++u) {
                const int i = tid + u * LMAZE_BLOCK;
                meta[u] = -1;
                va[u] = make_uint4(0u, 0u, 0u, 0u);
                vb[u] = make_uint4(0u, 0u, 0u, 0u);
                if (i >= items) continue;
                const int le = sb + i / IPE, r = i % IPE;
                const int w = r >= FOV ? 1 : 0, row = r - w * FOV;
                const int fl = flags[le];
                if (fl & (1 | 16 | 32)) continue;                           // untouched, or rewritten whole above
                const int cx = cen[le * 4], cy = cen[le * 4 + 1];
                const int wx = cen[le * 4 + 2 * w], wy = cen[le * 4 + 2 * w + 1];
                const int x = wx - 2 + row, y0 = wy - 2;
                if ((unsigned)x >= (unsigned)G) continue;                   // outside the array: stays 0
                // v5/v6: the record serves the previous window unless this call's update reaches into this row
                const bool touched = (fl & 128) && (unsigned)(x - cx + 2) <= 4u && (unsigned)(wy - cy + 4) <= 8u;
                if (V5 && w == 1 && (fl & 1024) && !touched) {
                    const int o = le * VPC + row * FOV;
                    struct __attribute__((packed, aligned(4))) Q4 { uint32_t v[4]; };
                    const Q4 q = *reinterpret_cast<const Q4*>(rec + o);
                    va[u] = make_uint4(q.v[0], q.v[1], q.v[2], q.v[3]);
                    vb[u].x = rec[o + 4];
                    meta[u] = o | (1 << 28);
                } else {
                    const int ty0 = y0 >> 2;                                // floor: -1 when the window pokes out on the left
                    const int o = (le * TILES + (x >> 2) * TB + ty0) * (VT * VT) + (x & 3) * VT;
                    const bool a_out = ty0 < 0, b_out = ty0 + 1 >= TB;
                    if (!a_out) va[u] = *reinterpret_cast<const uint4*>(vis + o);
                    if (!b_out) vb[u] = *reinterpret_cast<const uint4*>(vis + o + VT * VT);
                    meta[u] = (o & 0x0fffffff) | (a_out ? 1 << 29 : 0) | (b_out ? 1 << 30 : 0);
                }
            }
            __syncthreads();       // every load of this chunk's envs has returned before any of their cells is stored
#pragma unroll
            for (int u = 0; u < NIT; ++u) {
                if (meta[u] < 0) continue;
                const int i = tid + u * LMAZE_BLOCK;
                const int le = sb + i / IPE, r = i % IPE;
                const int w = r >= FOV ? 1 : 0, row = r - w * FOV;
                const int fl = flags[le], E0 = clk[le];
                const bool add = fl & 128, from_rec = (meta[u] >> 28) & 1;
                const int cx = cen[le * 4], cy = cen[le * 4 + 1];
                const int x = cen[le * 4 + 2 * w] - 2 + row, y0 = cen[le * 4 + 2 * w + 1] - 2;
                const int sh = from_rec ? 0 : (y0 & 3);
                // the eight words rotated so that the row's cells are c[0..4]
                uint32_t c[8] = {va[u].x, va[u].y, va[u].z, va[u].w, vb[u].x, vb[u].y, vb[u].z, vb[u].w};
                if (sh & 1) {
#pragma unroll
                    for (int k = 0; k < 7; ++k) c[k] = c[k + 1];
                }
                if (sh & 2) {
#pragma unroll
                    for (int k = 0; k < 6; ++k) c[k] = c[k + 2];
                }
                const bool rowc = (unsigned)(x - cx + 2) <= 4u;
                bool changed = false;
                float* out = vwin + le * 2 * W25 + w * W25 + row * FOV;
                const bool rec_out = V5 && (fl & (w == 0 ? 256 : 512));     // v5/v6: the record takes the window the NEXT call shows as previous
                // One cell: its true value under the clock this call ends with (a record holds true values, i.e. values stored
                // under clock VISIT_BIAS, and serves a row only when this call's update does not reach into it; a cell outside
                // the current window only takes the whole-plane halving of this call's update, if there is one).  `slow`: decode
                // by lmaze_visit_true (values that decayed below 2^-126) instead of the exponent subtraction.
                auto one_cell = [&](uint32_t& cj, int j, bool slow) -> bool {
                    const int y = y0 + j;
                    if ((unsigned)y >= (unsigned)G) return false;           // outside the array: stays 0
                    const bool in_cur = !from_rec && rowc && (unsigned)(y - cy + 2) <= 4u;
                    const int E = in_cur ? E0 : (from_rec ? VISIT_BIAS : E0) + (add ? 1 : 0);
                    const int n = E - VISIT_BIAS, f = (int)(cj >> 23);
                    const bool fast = cj == 0u || (f >= 1 && f - n >= 1);
                    uint32_t t = slow ? visit_true(cj, E) : (cj == 0u ? 0u : (uint32_t)((int)cj - n * (1 << 23)));
                    if (in_cur && add) {
                        const float nv = (__uint_as_float(t) + 1.0f) * 0.5f;    // v4:214; see lmaze_visit_add
                        t = __float_as_uint(nv);
                        if (fast || slow) cj = lmaze_visit_store(nv, E0 + 1);
                        changed = true;
                    }
                    out[j] = __uint_as_float(t);
                    if (rec_out) rec[le * VPC + row * FOV + j] = t;
                    return !fast;
                };
                uint32_t redo = 0u;
#pragma unroll
                for (int j = 0; j < FOV; ++j) redo |= one_cell(c[j], j, false) ? 1u << j : 0u;
#pragma unroll 1
                for (; redo; redo &= redo - 1u) {                           // rare: cells below 2^-126
                    const int j = __ffs((int)redo) - 1;
                    uint32_t cj = j == 0 ? c[0] : (j == 1 ? c[1] : (j == 2 ? c[2] : (j == 3 ? c[3] : c[4])));
                    one_cell(cj, j, true);
                    c[0] = j == 0 ? cj : c[0]; c[1] = j == 1 ? cj : c[1]; c[2] = j == 2 ? cj : c[2];
                    c[3] = j == 3 ? cj : c[3]; c[4] = j == 4 ? cj : c[4];
                }
                if (w == 0 && changed) {
                    // the updated words back where they came from: word k of the row sits at c[k - sh] for k >= sh
                    uint32_t d[8] = {va[u].x, va[u].y, va[u].z, va[u].w, vb[u].x, vb[u].y, vb[u].z, vb[u].w};
#pragma unroll
                    for (int k = 0; k < 8; ++k) {
#pragma unroll
                        for (int j = 0; j < FOV; ++j)
                            if (k - j >= 0 && k - j <= 3 && sh == k - j) d[k] = c[j];
                    }
                    const int o = meta[u] & 0x0fffffff;
                    if (!((meta[u] >> 29) & 1)) *reinterpret_cast<uint4*>(vis + o) = make_uint4(d[0], d[1], d[2], d[3]);
                    if (!((meta[u] >> 30) & 1)) *reinterpret_cast<uint4*>(vis + o + VT * VT) = make_uint4(d[4], d[5], d[6], d[7]);
                }
            }
            if (V5) {
                // rows of a new record that lie outside the array hold zeros
                for (int i = tid; i < items; i += LMAZE_BLOCK) {
                    const int le = sb + i / IPE, r = i % IPE;
                    const int w = r >= FOV ? 1 : 0, row = r - w * FOV;
                    const int fl = flags[le];
                    if ((fl & (1 | 16 | 32)) || !(fl & (w == 0 ? 256 : 512))) continue;
                    const int x = cen[le * 4 + 2 * w] - 2 + row, y0 = cen[le * 4 + 2 * w + 1] - 2;
                    for (int j = 0; j < FOV; ++j)
                        if ((unsigned)x >= (unsigned)G || (unsigned)(y0 + j) >= (unsigned)G) rec[le * VPC + row * FOV + j] = 0u;
                }
            }
          }
        }
        __syncthreads();
        if (V5) {
            // whole-map envs (reset / renormalised this call): their window values are in vwin now
            const int nd = ndense;
            for (int j = tid; j < nd * W25; j += LMAZE_BLOCK) {
                const int le = dlist[j / W25], k = j % W25, fl = flags[le];
                if (!(fl & (256 | 512))) continue;
                const int wsel = (fl & 256) ? 0 : 1;
                rec[le * VPC + k] = __float_as_uint(vwin[le * 2 * W25 + wsel * W25 + k]);
            }
        }
    }

    // ---------------- phase 3: render float[nb*C*25], contiguous, 16-byte stores ----------------
    // float `rem` of env le's observation: a bit of the string, or -- visit planes 2 and 6 of v4-v6, sampled live at
    // the current / "previous" window -- one of the env's 2 x 25 samples
    auto element = [&](int le, int rem) -> float {
        if (V4 && rem >= 2 * W25 && rem < 3 * W25) return vwin[le * 2 * W25 + rem - 2 * W25];
        if (V4 && rem >= 6 * W25) return vwin[le * 2 * W25 + rem - 5 * W25];
        const int f = le * PERENV + rem;
        return ((obits[f >> 5] >> (f & 31)) & 1u) ? 1.0f : 0.0f;
    };
    float* obs = a.b.obs + (size_t)blockbase * PERENV;
    const int R = (V5 && MODE == FM_PLANNER) ? 0 : nb * PERENV;   // plannerStep returns only the local observation
    // REC: the slot this step fills, or null (uniform over the workgroup).  The running obs is still written every step:
    // an env whose step is skipped (flag bit 0) keeps its previous observation, which the scalar path below copies from
    // there into the slot -- this workgroup stored it (an earlier step: the vmcnt(0) + barrier between steps) or it
    // predates the launch.  (Named only inside `if constexpr (REC)`: the plain forms keep their code.)
    const int nq = some_skipped ? 0 : (R >> 2);
    if (LMAZE_XP(a, 16) && !V4 && EPB == 128) {
        // experiment: the 4-KiB pieces of 8 consecutive workgroups interleaved (piece k*8 + w of the group's 1024
        // envs), content from this workgroup's own bit string (garbage addresses-wise)
        const int w = blockIdx.x & 7;
        float* gbase = a.b.obs + (size_t)(blockIdx.x >> 3) * 1024 * PERENV;
        const int npieces = 1024 * PERENV / 1024;
        for (int k = 0; k * 8 + w < npieces; ++k) {
            float v[4];
            nibble_floats(obits, (k * 256 + tid) % (EPB * PERENV / 4), v);
            typedef float v4f __attribute__((ext_vector_type(4)));
            v4f t = {v[0], v[1], v[2], v[3]};
            v4f* dst = reinterpret_cast<v4f*>(gbase) + (size_t)(k * 8 + w) * 256 + tid;
            if (a.nt) stream_store16(dst, t); else *dst = t;
        }
    }
    const int nq_run = (LMAZE_XP(a, 4) || (LMAZE_XP(a, 16) && !V4 && EPB == 128)) ? 0 : nq;
    for (int q = tid; q < nq_run; q += LMAZE_BLOCK) {
        const int f = q << 2;
        int le = f / PERENV;
        int rem = f - le * PERENV;
        float v[4];
        if (!V4) {
            // bit planes only (v1, v2): float f of the workgroup's range is bit f of the string phase 1 left in LDS,
            // a 16-byte store is nibble q of it -- a dozen VALU instructions per store, no index arithmetic
            // (masks per plane and a division per float made this loop ALU-bound: 1 210 VALU per wave on v2)
            nibble_floats(obits, q, v);
        } else {
            // v4-v6: five 0/1 planes and two float planes per env -- the nibble as above, then the floats that fall
            // into a visit plane are replaced by their samples (2 of 7 planes; a third of the stores touch one)
            nibble_floats(obits, q, v);
            if (rem + 3 >= 2 * W25 && !(rem >= 3 * W25 && rem + 3 < 6 * W25)) {
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    int r = rem + k, l2 = le;
                    if (r >= PERENV) { r -= PERENV; ++l2; }
                    if (r >= 2 * W25 && r < 3 * W25) v[k] = vwin[l2 * 2 * W25 + r - 2 * W25];
                    else if (r >= 6 * W25) v[k] = vwin[l2 * 2 * W25 + r - 5 * W25];
                }
            }
        }
        if (a.nt) {  // large batches: the observation cannot stay in the Infinity Cache, stream it (+6...12 %)
            typedef float v4f __attribute__((ext_vector_type(4)));
            v4f t = {v[0], v[1], v[2], v[3]};
            stream_store16(reinterpret_cast<v4f*>(obs) + q, t);
        } else {
            reinterpret_cast<float4*>(obs)[q] = make_float4(v[0], v[1], v[2], v[3]);
        }
        if constexpr (REC) {
            if (float* slot = roll_slot(ro, a.n, blockbase, t, PERENV)) roll_store4(ro, reinterpret_cast<float4*>(slot) + q, v);
        }
    }
    // scalar path: the ragged tail, or every element when some env of the workgroup is skipped
    for (int f = (nq << 2) + tid; f < R; f += LMAZE_BLOCK) {
        const int le = f / PERENV;
        if constexpr (REC) {
            if (float* slot = roll_slot(ro, a.n, blockbase, t, PERENV)) {
                if (flags[le] & 1) { slot[f] = obs[f]; continue; }    // skipped: the observation it keeps
                const float x = element(le, f - le * PERENV);
                obs[f] = x;
                slot[f] = x;
                continue;
            }
        }
        if (flags[le] & 1) continue;
        obs[f] = element(le, f - le * PERENV);
    }

    // ---------------- phase 3b (v5/v6): the local observation float[nb*4*25], v5:356-380 ----------------
    if (V5 && MODE != FM_RESET && !LMAZE_XP(a, 4)) {
        constexpr int PERLOC = 4 * W25;
        float* loc = a.b.obs_local + (size_t)blockbase * PERLOC;
        const int RL = nb * PERLOC;                      // 100 floats per env: a store never straddles two envs
        for (int q = tid; q < (RL >> 2); q += LMAZE_BLOCK) {
            const int f = q << 2;
            const int le = f / PERLOC;
            if constexpr (REC) {
                float* lslot = roll_lslot(ro, a.n, blockbase, t);
                if (lslot && (flags[le] & 1)) {          // skipped: the local observation it keeps
                    reinterpret_cast<float4*>(lslot)[q] = reinterpret_cast<const float4*>(loc)[q];
                    continue;
                }
            }
            if (flags[le] & 1) continue;
            float v[4];
            nibble_floats(lbits, q, v);
            if constexpr (REC) {
                if (float* lslot = roll_lslot(ro, a.n, blockbase, t)) roll_store4(ro, reinterpret_cast<float4*>(lslot) + q, v);
            }
            if (a.nt) {   // streamed like the foveal observation (round 3: these 400 B per env were plain stores)
                typedef float v4f __attribute__((ext_vector_type(4)));
                v4f t = {v[0], v[1], v[2], v[3]};
                stream_store16(reinterpret_cast<v4f*>(loc) + q, t);
            } else {
                reinterpret_cast<float4*>(loc)[q] = make_float4(v[0], v[1], v[2], v[3]);
            }
        }
    }
    if (ROLL && ++t < ro.T) {
        // rollout: the same chunk again.  Step t + 1 loads what step t stored, and not always in the same wave: a visit-tile
        // row or a v5/v6 window record is written by whichever lane held it this step.  So every wave waits here until its
        // global stores have completed (vmcnt(0); the compiler's own waits in front of the barrier below are for LDS only),
        // then the barrier: after it, any wave's loads see them -- the waves of one workgroup share this CU's vector L1,
        // which is write-through, so no cache invalidation is needed (the AMDGPU memory model's workgroup scope)
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    } else {
        t = 0;
        chunk += gridDim.x;
        if (chunk >= nchunks) break;                                       // uniform over the workgroup
        blockbase = chunk * EPB;
        nb = (int)min((int64_t)EPB, a.n - blockbase);
    }
    __syncthreads();                                                       // every wave is done with this chunk's strings and flags
    for (int i = tid; i < EPB * 12; i += LMAZE_BLOCK) obits[i] = 0u;
    if (V4) for (int i = tid; i < EPB * 2 * W25; i += LMAZE_BLOCK) vwin[i] = 0.0f;
    if (tid == 0) { any_skip = 0; ndense = 0; }
    __syncthreads();
  }
    if (warmed == 0x7fedcba9 && a.n < 0) a.b.done[0] = 1;   // never true: keeps the warming loads alive
#undef ROLL_ROW
#undef ROLL_EP
#undef LMAZE_POL
