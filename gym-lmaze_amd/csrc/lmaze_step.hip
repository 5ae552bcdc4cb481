// lmaze_step.hip -- the hot path: one kernel per step() of N independent mazes, gfx950.
//
// Replaces the body of the reference's step() (gym_lmaze/envs/lmaze_env.py:146-237,
// lmaze_env_v3.py:220-402): action decode, wall-collision check, position update,
// reward/done, and the full re-render of the observation planes.
//
// Shape of the work: per env 37 B of state traffic and 4*G*G B of
// observation written -- an HBM-write-bound stream with integer indexing, no MFMA.
//   phase 1  one lane per env: coalesced SoA loads, transition against the layout held in
//            LDS, coalesced SoA stores; the new ball cell goes to LDS.
//   phase 2  the workgroup's envs own one contiguous [envs*G*G] dword range of obs; lanes
//            stripe across it with 16-byte stores (1 KiB per wave instruction), so the
//            write is perfectly coalesced whatever G is.  Shared layout: the ball-free
//            pattern of a 16-byte-periodic group of envs is precomputed in LDS, so a
//            store costs one ds_read_b128 + a few compares.  Per-env layouts: the
//            workgroup's layouts are tiled into LDS first (one coalesced read), and both
//            the collision check and the render read them from there.
// Options folded into the same kernels (wave-uniform branches, no extra traffic):
//   auto_reset  an env whose done flag is set on entry is first re-placed exactly as
//               lmaze_reset(mask = done) would (reference reset(), lmaze_env.py:64-110)
//   mask        (observe only) re-render just the envs a masked reset touched
#include <cstdio>

#include <cmath>
#include <cstdlib>
#include <type_traits>

#include "lmaze_common.h"
#include "lmaze_learn.h"
#include "lmaze_policy_table.h"
#include "lmaze_rollout_lds.h"

namespace lmaze {

// Obs buffers larger than this are written with non-temporal stores: they cannot stay in the
// 256 MiB Infinity Cache anyway, and streaming them past L2 measured 0-7 % faster on MI355X;
// smaller buffers keep plain stores so the consumer of the observation finds them on-die.
static constexpr size_t kNonTemporalObsBytes = (size_t)192 << 20;

template <bool NT, int BITS = 0>
__device__ __forceinline__ void store16(int4* p, const int4& v) {
    typedef int v4i __attribute__((ext_vector_type(4)));
    if (NT) {
        v4i t = {v.x, v.y, v.z, v.w};
        stream_store16<BITS>(reinterpret_cast<v4i*>(p), t);
    } else {
        *p = v;
    }
}

// goalCount += 1 (v0:195) as an atomic without return: a plain read-modify-write makes the wave wait for the load --
// and with it for every load issued before, i.e. for the NEXT chunk's prefetched inputs -- whenever one of its 64 envs
// reaches the goal (about every second wave of a random rollout).  One lane per env, so the atomicity itself is unused.
__device__ __forceinline__ void count_goal(int32_t* p) { __hip_atomic_fetch_add(p, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// This launch's planes go beyond the caches (n envs of `cells` int32 cells each).
__host__ __device__ inline bool beyond_caches(int64_t n, int cells) { return (size_t)n * cells * 4 > kNonTemporalObsBytes; }

// One env's register state: the reference's per-env fields, this step's action and the done byte.  The done byte is
// the flag on entry as loaded (load_env) until env_advance replaces it with the step's own flag (0 / 1).
struct EnvState {
    int2 b, g;
    int act, sc, done;
    float r;
};

// One env's inputs, loaded into registers BEFORE the workgroup's LDS set-up and first barrier so
// that the two global round trips (layout, state) overlap instead of chaining: at launch-bound
// batch sizes (65 536 x 8x8) the kernel is nothing but that latency chain.
template <int VARIANT, bool DO_STEP>
__device__ __forceinline__ EnvState load_env(const StepArgs& a, int64_t e) {
    constexpr bool V3 = VARIANT == LMAZE_VARIANT_V3;
    EnvState in;
    in.b = a.ball[e];
    in.g = make_int2(-1, -1);
    if (V3) in.g = a.goal[e];
    in.act = 0; in.sc = 0; in.done = 0; in.r = 0.0f;
    if (DO_STEP) {
        in.act = a.action[e];
        in.sc = a.step_count[e];
        if (!V3) in.r = a.reward[e];
        // branch-free (a load under a branch is waited for where the branch ends, in front of whatever else is in flight):
        // without the fused reset the lane reads byte 0 of the layout instead -- one cached address, no traffic
        const uint8_t* dp = a.auto_reset ? a.done + e : a.layout;
        // ... and the byte is kept as loaded: every use is `a.auto_reset && in.done`.  A select here is a USE of the
        // loaded value inside the caller's `if (tid < nb)`: the wave then waits for its state loads before the set-up's
        // layout loads are even issued -- two global round trips in series at the head of every workgroup.
        in.done = *dp;
    }
    return in;
}

// reference reset() of one env (v0:64-110): the placement's cells (< 0: leave unchanged) and zeroed counters
template <int VARIANT>
__device__ __forceinline__ void env_reset(int ball_cell, int goal_cell, int G, EnvState& s) {
    if (ball_cell >= 0) s.b = make_int2(ball_cell / G, ball_cell % G);
    if (VARIANT == LMAZE_VARIANT_V3 && goal_cell >= 0) s.g = make_int2(goal_cell / G, goal_cell % G);
    s.sc = 0;      // v0:110
    s.r = -0.0f;   // v0:109
}

// the ball kept on the grid, as env_advance does first (the observe-only launches)
__device__ __forceinline__ void clamp_ball(EnvState& s, int G) { s.b = make_int2(clampi(s.b.x, 0, G - 1), clampi(s.b.y, 0, G - 1)); }

// reference step() of one env (v0:146-249, v3:220-402) on its register state; returns v0's goal hit (v0:195).
// cell_at(tx, ty) = the layout character of the target cell, from wherever the kernel keeps the layout.
template <int VARIANT, class CellAt>
__device__ __forceinline__ bool env_advance(const StepArgs& a, int G, CellAt cell_at, EnvState& s) {
    int bx = clampi(s.b.x, 0, G - 1), by = clampi(s.b.y, 0, G - 1);
    s.sc += 1;  // v0:151, v3:225
    int ox, oy;
    decode_action(s.act, ox, oy);
    const int tx = clampi(bx + ox, 0, G - 1), ty = clampi(by + oy, 0, G - 1);
    float r;
    bool dn;
    const bool hit = transition_rule<VARIANT>(a, cell_at(tx, ty), ox, oy, tx, ty, s.sc, s.r, s.g.x, s.g.y, bx, by, r, dn);
    s.b = make_int2(bx, by);
    s.r = r;
    s.done = dn ? 1 : 0;
    return hit;
}

// the per-env state a step kernel writes back
__device__ __forceinline__ void store_state(const StepArgs& a, int64_t e, const EnvState& s) {
    a.ball[e] = s.b;
    a.step_count[e] = s.sc;
    a.reward[e] = s.r;
    a.done[e] = s.done;
}

// cells of the planes' ball and goal bits; -8 = no goal (v0, or a v3 goal off the grid)
__device__ __forceinline__ int ball_cell_of(const int2& b, int G) { return b.x * G + b.y; }
template <int VARIANT>
__device__ __forceinline__ int goal_cell_of(const int2& g, int G) {
    return (VARIANT == LMAZE_VARIANT_V3 && g.x >= 0 && g.x < G && g.y >= 0 && g.y < G) ? g.x * G + g.y : -8;
}

// The reset epoch of a step launch, read at kernel start (a uniform load in front of every store: one scalar load):
// fetched where a done env draws its placement it was a global round trip inside phase 1 for every wave with a done
// env -- 90.0 instead of 83.4 us per step at 1M x 11x11 once the epoch lives on the device (captured rollouts)
__device__ __forceinline__ uint64_t step_epoch(const StepArgs& a, bool autoreset) {
    const uint64_t epoch = autoreset ? launch_epoch(a.epoch, a.epoch_in) : 0;
    if (autoreset) pass_epoch_on(a.epoch_in, a.epoch_out);
    return epoch;
}

// one env of phase 1 (layout in LDS); returns the env's ball (and goal) cell index for phase 2
// `place(draw, ball_cell, goal_cell)` = the fused reset's placement over the accepted cells (a list in LDS or bit masks)
template <int VARIANT, bool DO_STEP, class Place>
__device__ __forceinline__ void env_phase1(const StepArgs& a, const uint8_t* lay, int G, int64_t e, EnvState s,
                                           Place place, uint64_t epoch, int& ball_cell, int& goal_cell) {
    if (DO_STEP) {
        if (a.auto_reset && s.done) {
            int bc, gc;
            place(env_draw(a.seed, epoch, a.env_base + e), bc, gc);
            env_reset<VARIANT>(bc, gc, G, s);
            if (VARIANT == LMAZE_VARIANT_V3 && gc >= 0) a.goal_rw[e] = s.g;
        }
        if (env_advance<VARIANT>(a, G, [&](int tx, int ty) { return lay[tx * G + ty]; }, s) && a.goal_count)
            count_goal(a.goal_count + e);
        store_state(a, e, s);
    } else {
        clamp_ball(s, G);
    }
    ball_cell = ball_cell_of(s.b, G);
    goal_cell = goal_cell_of<VARIANT>(s.g, G);
}

// ------------------------------------------------------------------------------------
// Shared layout.  GT = G known at compile time (0: read it from the args);
// EPB = envs per workgroup (multiple of 4); NT = non-temporal obs stores.
// ------------------------------------------------------------------------------------
template <int GT, int VARIANT, bool DO_STEP, int EPB, bool NT>
__global__ __launch_bounds__(LMAZE_BLOCK) void step_shared_kernel(const StepArgs a) {
    constexpr bool V3 = VARIANT == LMAZE_VARIANT_V3;
    static_assert(EPB % 4 == 0 && EPB <= LMAZE_BLOCK, "group alignment; one lane per env");
    const int G = GT ? GT : a.grid;
    const int CELLS = G * G;
    // envs per 16-byte period of the obs stream: G even -> an env is a whole number of
    // 16-byte stores; G odd -> four envs are (G*G ints each, 4*G*G ints = G*G stores)
    const int GRP = (GT != 0 && (G & 1)) ? 4 : 1;
    const int PAT = (GT != 0) ? GRP * CELLS : CELLS;  // dwords of ball-free pattern kept in LDS

    extern __shared__ int4 lds4[];
    int* pat = reinterpret_cast<int*>(lds4);
    int* ballflat = pat + PAT;
    int* goalflat = ballflat + EPB;
    int* maskflag = goalflat + EPB;
    uint8_t* lay = reinterpret_cast<uint8_t*>(maskflag + EPB);
    uint16_t* spawn = reinterpret_cast<uint16_t*>(lay + ((CELLS + 15) & ~15));
    // v3, compile-time G: where the balls and goals are, as bit strings -- bit f of a group's string = dword f of the
    // group's GRP*G*G output dwords holds one -- so that a 16-byte store ORs two nibbles into its pattern instead of
    // comparing eight indices with four positions (v3's render loop was ~100 VALU instructions per store: 1M x 11x11
    // 94-97 us, 77-79 with the strings; 512K x 18x18 109 -> 103-109).  v0 keeps the comparisons: the strings give the same
    // best time there (76.7-78.9 us) but only at narrow launch policies -- its extra VALU work paces the stores about right
    // ("a wait that staggers").  Two buffers, used by alternate chunks.
    constexpr bool MARKS = GT != 0 && V3;
    constexpr int GRPT = (GT & 1) ? 4 : 1, NPL = V3 ? 2 : 1;
    constexpr int WPG = GT ? (GRPT * GT * GT + 31) / 32 : 1;      // words per group string
    constexpr int NGW = GT ? (EPB / GRPT) * WPG : 1;              // words per plane
    uint32_t* marks = reinterpret_cast<uint32_t*>(reinterpret_cast<uint8_t*>(spawn) + ((CELLS * 2 + 15) & ~15));   // [2][NPL][NGW]
    __shared__ int spawn_count_s;

    const int tid = threadIdx.x;
    if (MARKS)
        for (int i = tid; i < 2 * NPL * NGW; i += LMAZE_BLOCK) marks[i] = 0u;
    // A workgroup takes chunks of EPB envs grid-stride (chunk = blockIdx.x, + gridDim.x, ...): with one chunk
    // each (gridDim.x = number of chunks) it is the plain one-chunk kernel; with several, the inputs of the
    // NEXT chunk are loaded while the current one is being stored, so their latency -- several microseconds
    // when they miss the caches and queue behind a saturated write stream -- is no longer exposed with only
    // 3 workgroups resident per CU.  Consecutive workgroups still write consecutive chunks at any moment.
    const int64_t nchunks = (a.n + EPB - 1) / EPB;
    int64_t chunk = blockIdx.x;
    int64_t blockbase = chunk * EPB;
    int nb = (int)min((int64_t)EPB, a.n - blockbase);  // envs of the current chunk
    const bool masked = !DO_STEP && a.mask != nullptr;
    const bool autoreset = DO_STEP && a.auto_reset;
    // step_epoch() written out: through the helper this kernel's set-up compiles to other branches and waits
    const uint64_t epoch = autoreset ? launch_epoch(a.epoch, a.epoch_in) : 0;
    if (autoreset) pass_epoch_on(a.epoch_in, a.epoch_out);

    EnvState in{};
    if (tid < nb) in = load_env<VARIANT, DO_STEP>(a, blockbase + tid);
    // Streaming regime without the fused reset: the state loads are waited for BEFORE the set-up's layout loads go out.
    // That is a second round trip in series at the head of every workgroup, and it is faster: 1M x 11x11 at the default
    // policy 76.1-78.2 us on three boxes with it, 85-93 without (then only a narrow (5, 1) / (4, 2) reaches 77) --
    // the pause staggers the workgroups of a CU, fewer of them stream their ranges at the same moment (the regime
    // DESIGN 5.3 describes).  With the fused reset the set-up is longer and staggers by itself: 78.5-83 us without
    // the wait against 84-86 with it.  (Found when the done flag's `auto_reset ? byte : 0` select -- a use of a loaded
    // value inside the branch above -- turned out to have been that wait all along.)
    // It is a STAGGER, nothing else, and it is kept only while it pays: launch_hint bit 9 switches it off, and the guard
    // test times both (tests/test_gpu_policy_guard.py).
    if (DO_STEP && NT && !autoreset && !(a.launch_hint & 0x200)) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");

    // Large batches (NT): the first 256 workgroups touch every 64-byte line of this step's action row at kernel
    // start -- ONE burst of reads before the write stream saturates -- so that the chunk loads later in the
    // launch find the row in the memory-side cache.  Actions are the one input that is new every step (state
    // was written by the previous step and is still cached): read chunk by chunk from HBM they are 4 of 521
    // bytes per env but cost 17-25 % of the rate, each small read turning a saturated write stream around
    // (1M x 11x11, a fresh action row per step, 3 workgroups per CU x 2 chunks: 108 us without, 85-86 with;
    // 86 us when the rows are cache-resident anyway).
    // The same for the per-env state, which is only cached if nothing else ran since the previous step: with a
    // 512-MB copy between two steps (a stand-in for a policy network) the step took 131 us instead of 83.
    // Written out here and in step_shared_u8_kernel, not as a shared helper: through one, this kernel's set-up compiled
    // to other branches and waited for one more load (vmcnt(0) instead of vmcnt(1)) before its first chunk.
    int warmed = 0;
    if (DO_STEP && NT) {
        warmed = warm_lines(a.action, a.n * 4, 256) + warm_lines(a.ball, a.n * 8, 256) +
                 warm_lines(a.step_count, a.n * 4, 256);
        if (!V3) warmed += warm_lines(a.reward, a.n * 4, 256);
        if (V3) warmed += warm_lines(a.goal, a.n * 8, 256);
        if (autoreset) warmed += warm_lines(a.done, a.n, 256);
    }

    constexpr int NSM = GT ? (GT * GT + 63) / 64 : 1;
    unsigned long long okm[NSM] = {};                             // GT != 0: accepted spawn cells, 64 per word
    int okcount = 0;
    if (GT != 0) {
        // Set-up with ONE global round trip: every layout byte this lane needs -- its cells for the LDS copy and the
        // pattern, and (wave 0, fused reset) the cells it ranks for the spawn list -- is loaded into registers before
        // the first is used.  Written as plain loops the compiler waits for each load where it is consumed: layout,
        // pattern, spawn list chunk 1, chunk 2 = four L2 round trips in series in front of the workgroup's first
        // barrier (two without the fused reset), about 0.5 us each with only 3 workgroups per CU to hide them.
        constexpr int CG = (GT ? GT : 1) * (GT ? GT : 1), NL = (CG + LMAZE_BLOCK - 1) / LMAZE_BLOCK, NS = (CG + 63) / 64;
        uint8_t cb[NL], sb[NS];
#pragma unroll
        for (int j = 0; j < NL; ++j) {
            cb[j] = a.layout[min(tid + j * LMAZE_BLOCK, CG - 1)];     // unconditional (clamped): a load under a branch is
        }                                                             // waited for where the branch ends
        if (autoreset) {                                              // uniform
#pragma unroll
            for (int j = 0; j < NS; ++j) sb[j] = a.layout[min((tid & 63) + j * 64, CG - 1)];
        }
#pragma unroll
        for (int j = 0; j < NL; ++j) {
            const int c = tid + j * LMAZE_BLOCK;
            if (c < CG) {
                lay[c] = cb[j];
                const int bits = cell_bits<VARIANT>(cb[j]);
                for (int g = 0; g < GRP; ++g) pat[g * CG + c] = bits;
            }
        }
        if (autoreset) {
            // the accepted spawn cells as NS ballots, bit c of the string = cell c accepted: every wave ranks the same
            // bytes, so the masks are wave-uniform scalars and nothing goes through LDS.  (Round 2: as a compacted
            // list built by wave 0 in front of the barrier the fused reset cost 4.7 of 83 us at 1M x 11x11 even
            // when no env was done -- the list is only read by the few lanes that reset.)
#pragma unroll
            for (int j = 0; j < NS; ++j) {
                const int c = (tid & 63) + j * 64;
                okm[j] = __ballot(c < CG && interior(c, G) && spawn_ok<VARIANT>(sb[j]));
                okcount += __popcll(okm[j]);
            }
        }
    } else {
        for (int i = tid; i < CELLS; i += LMAZE_BLOCK) lay[i] = a.layout[i];
        for (int i = tid; i < PAT; i += LMAZE_BLOCK) pat[i] = cell_bits<VARIANT>(a.layout[i]);
        if (autoreset && tid < 64) {
            const int cnt = wave_build_spawn_list<VARIANT>(a.layout, G, CELLS, spawn, tid);
            if (tid == 0) spawn_count_s = cnt;
        }
    }
    __syncthreads();

  int buf = 0;
  for (;;) {
    const int64_t next = chunk + gridDim.x;
    const bool has_next = next < nchunks;                         // uniform over the workgroup
    uint32_t* mk = marks + buf * NPL * NGW;
    EnvState in_next{};
    int nb_next = 0;
    if (has_next) {                                               // issued now, consumed one chunk later
        nb_next = (int)min((int64_t)EPB, a.n - next * EPB);
        if (tid < nb_next) in_next = load_env<VARIANT, DO_STEP>(a, next * EPB + tid);
    }

    if (tid < EPB) {  // one lane per env
        const int le = tid;
        int bf = -8, gf = -8, mf = 0;
        if (le < nb) {
            const int64_t e = blockbase + le;
            int bc, gc;
            if (GT != 0) {
                env_phase1<VARIANT, DO_STEP>(a, lay, G, e, in, [&](uint4 d, int& pb, int& pg) { place_from_masks<VARIANT, NSM>(okm, okcount, d, pb, pg); }, epoch, bc, gc);
            } else {
                const int cnt = autoreset ? spawn_count_s : 0;
                env_phase1<VARIANT, DO_STEP>(a, lay, G, e, in, [&](uint4 d, int& pb, int& pg) { place_from_list<VARIANT>(spawn, cnt, d, pb, pg); }, epoch, bc, gc);
            }
            const int off = (GT != 0) ? (le % GRP) * CELLS : 0;
            bf = off + bc;
            if (V3 && gc >= 0) gf = off + gc;
            if (masked) mf = a.mask[e] != 0;
            if (MARKS) {
                const int gi = (le / GRP) * WPG;
                atomicOr(&mk[gi + (bf >> 5)], 1u << (bf & 31));
                if (V3 && gc >= 0) atomicOr(&mk[NGW + gi + (gf >> 5)], 1u << (gf & 31));
            }
        }
        ballflat[le] = bf;
        if (V3) goalflat[le] = gf;
        if (masked) maskflag[le] = mf;
    }
    if (a.obs != nullptr) {
    __syncthreads();

    int32_t* obs = a.obs + (size_t)blockbase * CELLS;
    int4* obs4 = reinterpret_cast<int4*>(obs);
    const int R = nb * CELLS;  // dwords this workgroup writes
    const int nq = R >> 2;     // whole 16-byte stores

    if (GT != 0) {
        const int V4G = PAT >> 2;  // stores per group of GRP envs
        const int4* pat4 = reinterpret_cast<const int4*>(pat);
        if (MARKS && has_next)                                    // the other buffer, for the next chunk's phase 1
            for (int i = tid; i < NPL * NGW; i += LMAZE_BLOCK) marks[(buf ^ 1) * NPL * NGW + i] = 0u;
        for (int q = tid; q < nq; q += LMAZE_BLOCK) {
            const int grp = q / V4G;
            const int p = q - grp * V4G;
            int4 v = pat4[p];
            const int p4 = p << 2;
            if (masked) {
                if (GRP == 4) {
                    const int4 m = reinterpret_cast<const int4*>(maskflag)[grp];
                    if (!(m.x | m.y | m.z | m.w)) continue;
                } else if (!maskflag[grp]) {
                    continue;
                }
            }
            if (MARKS) {
                // dwords 4p .. 4p+3 of the group: one nibble of each string (4 divides 32: never across two words)
                const int w = grp * WPG + (p4 >> 5), sh = p4 & 31;
                const uint32_t b4 = mk[w] >> sh, g4 = mk[NGW + w] >> sh;
                v.x |= (int)(b4 & 1u) * LMAZE_OBS_BALL | (int)(g4 & 1u) * LMAZE_OBS_GOAL;
                v.y |= (int)((b4 >> 1) & 1u) * LMAZE_OBS_BALL | (int)((g4 >> 1) & 1u) * LMAZE_OBS_GOAL;
                v.z |= (int)((b4 >> 2) & 1u) * LMAZE_OBS_BALL | (int)((g4 >> 2) & 1u) * LMAZE_OBS_GOAL;
                v.w |= (int)((b4 >> 3) & 1u) * LMAZE_OBS_BALL | (int)((g4 >> 3) & 1u) * LMAZE_OBS_GOAL;
            } else if (GRP == 4) {
                const int4 bf = reinterpret_cast<const int4*>(ballflat)[grp];
                or_at(v, bf.x - p4, LMAZE_OBS_BALL);
                or_at(v, bf.y - p4, LMAZE_OBS_BALL);
                or_at(v, bf.z - p4, LMAZE_OBS_BALL);
                or_at(v, bf.w - p4, LMAZE_OBS_BALL);
            } else {
                or_at(v, ballflat[grp] - p4, LMAZE_OBS_BALL);
            }
            store16<NT>(obs4 + q, v);
        }
    } else {
        for (int q = tid; q < nq; q += LMAZE_BLOCK) {
            const int f0 = q << 2;
            int le = f0 / CELLS;
            int c = f0 - le * CELLS;
            if (masked) {  // the store may straddle two envs
                const int le1 = (f0 + 3) / CELLS;
                if (!(maskflag[le] | maskflag[le1 < EPB ? le1 : le])) continue;
            }
            int vals[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                int v = pat[c];
                v |= (ballflat[le] == c) ? LMAZE_OBS_BALL : 0;
                if (V3) v |= (goalflat[le] == c) ? LMAZE_OBS_GOAL : 0;
                vals[j] = v;
                if (++c == CELLS) { c = 0; ++le; }
            }
            store16<NT>(obs4 + q, make_int4(vals[0], vals[1], vals[2], vals[3]));
        }
    }
    // ragged tail (last workgroup only, when nb*G*G is not a multiple of 4)
    const int f = (nq << 2) + tid;
    if (f < R) {
        const int le = f / CELLS;
        const int c = f - le * CELLS;
        const int off = (GT != 0) ? (le % GRP) * CELLS : 0;
        int v = pat[(GT != 0 && GRP > 1) ? off + c : c];
        v |= (ballflat[le] == off + c) ? LMAZE_OBS_BALL : 0;
        if (V3) v |= (goalflat[le] == off + c) ? LMAZE_OBS_GOAL : 0;
        if (!masked || maskflag[le]) obs[f] = v;
    }
    }  // obs != nullptr
    if (!has_next) break;
    __syncthreads();   // the per-env cells in LDS are rewritten by the next chunk's phase 1
    chunk = next;
    blockbase = chunk * EPB;
    nb = nb_next;
    in = in_next;
    buf ^= 1;
  }
  if (warmed == 0x7fedcba9 && a.n < 0) a.done[0] = 1;   // never true: keeps the warming loads alive
}

// ------------------------------------------------------------------------------------
// Per-env layouts: uint8[N,G,G] in HBM, tiled into LDS per workgroup.
// ------------------------------------------------------------------------------------
template <int GT, int VARIANT, bool DO_STEP>
__global__ __launch_bounds__(LMAZE_BLOCK) void step_perenv_kernel(const StepArgs a) {
    constexpr bool V3 = VARIANT == LMAZE_VARIANT_V3;
    const int G = GT ? GT : a.grid;
    const int CELLS = G * G;
    const int EPB = a.envs_per_block;  // multiple of 16: keeps the tile base 16-byte aligned

    extern __shared__ int4 lds4[];
    uint8_t* tile = reinterpret_cast<uint8_t*>(lds4);  // [EPB*CELLS] layouts of this workgroup
    const int tile_bytes = (EPB * CELLS + 15) & ~15;
    int* ballcell = reinterpret_cast<int*>(tile + tile_bytes);  // [EPB+1]
    int* goalcell = ballcell + EPB + 1;                         // [EPB+1]
    int* flag = goalcell + EPB + 1;                             // [EPB+1] done-on-entry / observe mask
    int* newball = flag + EPB + 1;                              // [EPB]   auto-reset placement
    int* newgoal = newball + EPB;                               // [EPB]

    const int tid = threadIdx.x;
    const int64_t blockbase = (int64_t)blockIdx.x * EPB;
    const int nb = (int)min((int64_t)EPB, a.n - blockbase);
    const int R = nb * CELLS;  // layout bytes read == obs dwords written by this workgroup
    const bool autoreset = DO_STEP && a.auto_reset;
    const bool masked = !DO_STEP && a.mask != nullptr;
    const uint64_t epoch = step_epoch(a, autoreset);

    EnvState s{};  // this lane's env, loaded while the layouts are still on their way
    if (tid < nb) s = load_env<VARIANT, DO_STEP>(a, blockbase + tid);
    if (tid <= EPB) {
        int f = 0;
        if (tid < nb) {
            if (autoreset) f = s.done != 0;
            if (masked) f = a.mask[blockbase + tid] != 0;
        }
        flag[tid] = f;
    }
    // stage the layouts: 16 B per lane per instruction, ragged byte tail
    const uint8_t* src = a.layout + (size_t)blockbase * CELLS;
    const int n16 = R >> 4;
    for (int i = tid; i < n16; i += LMAZE_BLOCK) lds4[i] = reinterpret_cast<const int4*>(src)[i];
    for (int i = (n16 << 4) + tid; i < R; i += LMAZE_BLOCK) tile[i] = src[i];
    __syncthreads();

    if (autoreset) {
        // wave w re-places the done envs w, w+4, ... of the workgroup with ballot scans of their tiles
        const int lane = tid & 63;
        for (int le = tid >> 6; le < nb; le += LMAZE_BLOCK / 64) {
            if (!flag[le]) continue;
            int bc, gc;
            wave_place<VARIANT>(tile + le * CELLS, G, CELLS, env_draw(a.seed, epoch, a.env_base + blockbase + le), lane,
                                bc, gc);
            if (lane == 0) { newball[le] = bc; newgoal[le] = gc; }
        }
        __syncthreads();
    }

    if (tid <= EPB) {
        int bcell = -8, gcell = -8;
        if (tid < nb) {
            const int64_t e = blockbase + tid;
            if (DO_STEP) {
                if (autoreset && flag[tid]) {
                    const int gc = newgoal[tid];
                    env_reset<VARIANT>(newball[tid], gc, G, s);
                    if (V3 && gc >= 0) a.goal_rw[e] = s.g;
                }
                if (env_advance<VARIANT>(a, G, [&](int tx, int ty) { return tile[tid * CELLS + tx * G + ty]; }, s) && a.goal_count)
                    count_goal(a.goal_count + e);
                store_state(a, e, s);
            } else {
                clamp_ball(s, G);
            }
            bcell = ball_cell_of(s.b, G);
            gcell = goal_cell_of<VARIANT>(s.g, G);
        }
        ballcell[tid] = bcell;
        if (V3) goalcell[tid] = gcell;
    }
    if (a.obs == nullptr) return;
    // large batches: non-temporal stores, as in the other kernels (1M x 11x11 per-env layouts, 8-KiB tiles: 121 -> 102 us)
    const bool stream = beyond_caches(a.n, CELLS);   // uniform
    __syncthreads();

    int32_t* obs = a.obs + (size_t)blockbase * CELLS;
    int4* obs4 = reinterpret_cast<int4*>(obs);
    const int nq = R >> 2;
    const uint32_t* tile32 = reinterpret_cast<const uint32_t*>(tile);
    const bool whole = (CELLS & 3) == 0;  // a 16-byte store never straddles two envs
    for (int q = tid; q < nq; q += LMAZE_BLOCK) {
        const uint32_t w = tile32[q];  // 4 layout cells
        const int f0 = q << 2;
        int le = f0 / CELLS;
        int c = f0 - le * CELLS;
        int vals[4];
        if (whole) {
            if (masked && !flag[le]) continue;
            const int bc = ballcell[le] - c;
            const int gc = V3 ? goalcell[le] - c : -8;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                int v = cell_bits<VARIANT>((uint8_t)(w >> (8 * j)));
                v |= (bc == j) ? LMAZE_OBS_BALL : 0;
                if (V3) v |= (gc == j) ? LMAZE_OBS_GOAL : 0;
                vals[j] = v;
            }
        } else {
            if (masked && !(flag[le] | flag[(f0 + 3) / CELLS])) continue;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                int v = cell_bits<VARIANT>((uint8_t)(w >> (8 * j)));
                v |= (ballcell[le] == c) ? LMAZE_OBS_BALL : 0;
                if (V3) v |= (goalcell[le] == c) ? LMAZE_OBS_GOAL : 0;
                vals[j] = v;
                if (++c == CELLS) { c = 0; ++le; }
            }
        }
        if (stream) store16<true>(obs4 + q, make_int4(vals[0], vals[1], vals[2], vals[3]));
        else obs4[q] = make_int4(vals[0], vals[1], vals[2], vals[3]);
    }
    const int f = (nq << 2) + tid;
    if (f < R) {
        const int le = f / CELLS;
        const int c = f - le * CELLS;
        int v = cell_bits<VARIANT>(tile[f]);
        v |= (ballcell[le] == c) ? LMAZE_OBS_BALL : 0;
        if (V3) v |= (goalcell[le] == c) ? LMAZE_OBS_GOAL : 0;
        if (!masked || flag[le]) obs[f] = v;
    }
}

// ------------------------------------------------------------------------------------
// Per-env layouts, register-tiled: one WAVE per env, no LDS, no barrier (G*G a multiple of
// 256: G = 16, 32, 48, 64).  Lane l loads dword 64*j + l of the env's layout (256 B per wave
// instruction, each byte read from HBM once) and keeps it in registers; the target cell of
// the transition is fetched with v_readlane; every quantity of the transition is
// wave-uniform, lane 0 stores it; the lane's 4 cells per register become one 16-byte store,
// so every wave store instruction writes 1 KiB contiguous.  Waves never wait for each other.
// The one kernel that spells out the transition (env_reset, env_advance, store_state, the cell helpers, step_epoch)
// itself: through the shared helpers -- any subset of them -- its registers were allocated differently, 71 instead of
// 69 VGPRs at G = 32 (v0) and 83 instead of 79 (v3, one wave per SIMD fewer).  A change of the rule lands here too.
// ------------------------------------------------------------------------------------
template <int G, int VARIANT, bool DO_STEP, bool NT>
__global__ __launch_bounds__(LMAZE_BLOCK) void step_perenv_wave_kernel(const StepArgs a) {
    constexpr bool V3 = VARIANT == LMAZE_VARIANT_V3;
    constexpr int CELLS = G * G, NJ = CELLS / 256;
    static_assert(CELLS % 256 == 0, "whole dwords per lane");
    const int lane = threadIdx.x & 63;
    const int EPW = a.envs_per_block;  // envs per wave
    const int64_t wave = (int64_t)blockIdx.x * (LMAZE_BLOCK / 64) + (threadIdx.x >> 6);
    const bool autoreset = DO_STEP && a.auto_reset;
    const bool masked = !DO_STEP && a.mask != nullptr;
    // the reset epoch at kernel start, as step_epoch()
    const uint64_t epoch = autoreset ? launch_epoch(a.epoch, a.epoch_in) : 0;
    if (autoreset) pass_epoch_on(a.epoch_in, a.epoch_out);

#pragma unroll 1
    for (int k = 0; k < EPW; ++k) {
        const int64_t e = wave * EPW + k;
        if (e >= a.n) break;
        if (masked && !a.mask[e]) continue;
        const uint32_t* lay32 = reinterpret_cast<const uint32_t*>(a.layout + (size_t)e * CELLS);
        uint32_t w[NJ];
#pragma unroll
        for (int j = 0; j < NJ; ++j) w[j] = lay32[j * 64 + lane];

        int2 b = a.ball[e];
        int2 g = make_int2(-1, -1);
        if (V3) g = a.goal[e];
        if (DO_STEP) {
            const int act = a.action[e];
            int sc_in = a.step_count[e];
            float r_in = V3 ? 0.0f : a.reward[e];
            if (autoreset && a.done[e]) {  // re-place from the layout registers (wave-uniform branch)
                int bc, gc;
                wave_place_regs<VARIANT, G, NJ>(w, env_draw(a.seed, epoch, a.env_base + e), lane, bc, gc);
                if (bc >= 0) b = make_int2(bc / G, bc % G);
                if (V3 && gc >= 0) {
                    g = make_int2(gc / G, gc % G);
                    if (lane == 0) a.goal_rw[e] = g;
                }
                sc_in = 0;
                r_in = -0.0f;
            }
            int bx = clampi(b.x, 0, G - 1), by = clampi(b.y, 0, G - 1);
            int ox, oy;
            decode_action(act, ox, oy);
            const int tx = clampi(bx + ox, 0, G - 1), ty = clampi(by + oy, 0, G - 1);
            const int t = __builtin_amdgcn_readfirstlane(tx * G + ty);  // wave-uniform by construction
            const int tw = t >> 2;                                      // dword of the layout holding the target cell
            uint32_t word = 0;
#pragma unroll
            for (int j = 0; j < NJ; ++j)
                if ((tw >> 6) == j) word = __builtin_amdgcn_readlane(w[j], tw & 63);
            const uint8_t c = (uint8_t)(word >> (8 * (t & 3)));
            float r;
            bool dn;
            const int sc = sc_in + 1;
            const bool hit = transition_rule<VARIANT>(a, c, ox, oy, tx, ty, sc, r_in, g.x, g.y, bx, by, r, dn);
            if (lane == 0) {
                if (hit && a.goal_count) count_goal(a.goal_count + e);
                a.ball[e] = make_int2(bx, by);
                a.step_count[e] = sc;
                a.reward[e] = r;
                a.done[e] = dn ? 1 : 0;
            }
            b = make_int2(bx, by);
        } else {
            b = make_int2(clampi(b.x, 0, G - 1), clampi(b.y, 0, G - 1));
        }
        if (a.obs == nullptr) continue;
        const int bcell = b.x * G + b.y;
        const int gcell = (V3 && g.x >= 0 && g.x < G && g.y >= 0 && g.y < G) ? g.x * G + g.y : -8;
        int4* obs4 = reinterpret_cast<int4*>(a.obs + (size_t)e * CELLS);
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            const int c0 = (j * 64 + lane) << 2;  // first of this lane's 4 cells
            int vals[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                int v = cell_bits<VARIANT>((uint8_t)(w[j] >> (8 * q)));
                v |= (bcell == c0 + q) ? LMAZE_OBS_BALL : 0;
                if (V3) v |= (gcell == c0 + q) ? LMAZE_OBS_GOAL : 0;
                vals[q] = v;
            }
            store16<NT, 2>(obs4 + j * 64 + lane, make_int4(vals[0], vals[1], vals[2], vals[3]));   // `sc0 sc1 nt`: -5.6 % here (lmaze_common.h)
        }
    }
}

// ------------------------------------------------------------------------------------
// Shared 8x8 layout, small batches (BASELINE config 2: 65 536 x 8x8, 16.8 MB of planes): wave-autonomous.
// At this size a launch is nothing but a latency chain -- 5.7-6.0 us per step against 4.6 us for a bare fill
// of the same bytes -- so the chain is cut to its minimum: no LDS, no workgroup barrier.  One wave = 64 envs;
// lane l holds the layout byte of cell l (the 64 cells ARE the wave), so the transition's target cell and the
// render's pattern come from other lanes by ds_bpermute; the wave's 64 x 256 B of planes are one contiguous
// 16 KiB, 16 stores per lane, store k of lane l covering cells 4(l % 16)..+3 of env l/16 + 4k -- the pattern
// int4 is loop-invariant per lane.  Fused auto-reset: the accepted spawn cells are a 64-bit ballot.
// ------------------------------------------------------------------------------------

// EPW = envs per wave (64, 32 or 16: fewer envs per wave = more, shorter waves to hide the load latency with)
// Tried and dropped (round 2): storing the ball-free planes first -- they need the 64-byte layout only -- and
// patching the ball cell's dword once the inputs have arrived, to hide the load latency behind the stores: 6.5-7.7 us
// instead of 5.6 (one partial-line store per env costs more than the latency it hides).
template <int VARIANT, bool DO_STEP, int EPW>
__global__ __launch_bounds__(LMAZE_BLOCK) void step_shared_wave8_kernel(const StepArgs a) {
    constexpr bool V3 = VARIANT == LMAZE_VARIANT_V3;
    constexpr int G = 8, CELLS = 64;
    const int lane = threadIdx.x & 63;
    // blockDim.x / 64 autonomous waves per workgroup (no barrier, no LDS: the grouping only changes what the dispatcher sees)
    const int64_t base = ((int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6)) * EPW;
    if (base >= a.n) return;
    const int nb = (int)min((int64_t)EPW, a.n - base);
    const bool autoreset = DO_STEP && a.auto_reset;
    const uint64_t epoch = step_epoch(a, autoreset);
    const bool live = lane < nb;
    const int myc = a.layout[lane];                                   // cell `lane` of the layout; issued first
    EnvState s{};
    s.b = make_int2(1, 1); s.g = make_int2(-1, -1);
    if (live) s = load_env<VARIANT, DO_STEP>(a, base + lane);
    const int mypat = cell_bits<VARIANT>((uint8_t)myc);
    const int p4 = (lane & 15) << 2;                                  // first cell of this lane's stores
    const int4 pat4 = make_int4(__shfl(mypat, p4, 64), __shfl(mypat, p4 + 1, 64), __shfl(mypat, p4 + 2, 64),
                                __shfl(mypat, p4 + 3, 64));
    int4* obs4 = reinterpret_cast<int4*>(a.obs + (size_t)base * CELLS);
    if (DO_STEP) {
        if (autoreset) {   // placement over the accepted cells of the wave's 64, one ballot
            const unsigned long long ok[1] = {__ballot(interior(lane, G) && spawn_ok<VARIANT>((uint8_t)myc))};
            if (s.done) {
                int bc, gc;
                place_from_masks<VARIANT, 1>(ok, __popcll(ok[0]), env_draw(a.seed, epoch, a.env_base + base + lane), bc, gc);
                env_reset<VARIANT>(bc, gc, G, s);
                if (V3 && gc >= 0 && live) a.goal_rw[base + lane] = s.g;
            }
        }
        // v0:172, v3:251 -- every lane takes part in the __shfl
        const bool hit = env_advance<VARIANT>(a, G, [&](int tx, int ty) { return (uint8_t)__shfl(myc, tx * G + ty, 64); }, s);
        if (live) {
            const int64_t e = base + lane;
            if (hit && a.goal_count) count_goal(a.goal_count + e);
            store_state(a, e, s);
        }
    } else {
        clamp_ball(s, G);
    }
    if (a.obs == nullptr) return;
    const int ball_cell = ball_cell_of(s.b, G);
    const int goal_cell = goal_cell_of<VARIANT>(s.g, G);
#pragma unroll
    for (int k = 0; k < EPW / 4; ++k) {
        const int le = (lane >> 4) + 4 * k;                           // env of store k
        const int bc = __shfl(ball_cell, le, 64);
        const int gc = V3 ? __shfl(goal_cell, le, 64) : -8;
        int4 v = pat4;
        or_at(v, bc - p4, LMAZE_OBS_BALL);
        if (V3) or_at(v, gc - p4, LMAZE_OBS_GOAL);
        if (le < nb) obs4[lane + 64 * k] = v;
    }
}

// ------------------------------------------------------------------------------------
// Narrow observation: the same bit mask in ONE BYTE per cell, uint8[N,G,G] -- the mask needs four
// bits --, 37 + G*G bytes per env-step instead of 37 + 4 G*G (11x11: 158 against 521).  The int32 planes stay the
// metric's mode; this is a separate workload with its own algorithmic bytes.  Shared layout, any G.
// Phase 1 is the int32 kernel's (env_phase1); the render stripes the workgroup's EPB * G*G bytes with 16-byte stores,
// 16 cells each, which straddle envs at every odd G: the static pattern comes from four byte-shifted copies of the
// layout's bits laid out twice in a row (so that any 16 consecutive cells, wrapping into the next env, are four aligned
// dword reads), the ball / goal bytes of the one or two envs a store touches are OR-ed in.
// ------------------------------------------------------------------------------------
template <int VARIANT, bool DO_STEP, int EPB>
__global__ __launch_bounds__(LMAZE_BLOCK) void step_shared_u8_kernel(const StepArgs a) {
    constexpr bool V3 = VARIANT == LMAZE_VARIANT_V3;
    static_assert(EPB % 16 == 0 && EPB <= LMAZE_BLOCK, "a workgroup's byte range starts on a 16-byte boundary; one lane per env");
    const int G = a.grid, CELLS = G * G;
    const int PW = (2 * CELLS + 16 + 3) >> 2;             // dwords of one shifted copy: the pattern twice + 16 bytes of slack
    extern __shared__ int4 lds4[];
    uint32_t* patw = reinterpret_cast<uint32_t*>(lds4);                 // [4][PW] copy s = the doubled pattern starting at byte s
    int* ballflat = reinterpret_cast<int*>(patw + 4 * PW);              // [EPB + 1]
    int* goalflat = ballflat + EPB + 1;                                 // [EPB + 1]
    int* maskflag = goalflat + EPB + 1;                                 // [EPB + 1]
    uint16_t* spawn = reinterpret_cast<uint16_t*>(maskflag + EPB + 1);  // [CELLS]
    uint8_t* lay = reinterpret_cast<uint8_t*>(spawn + ((CELLS + 1) & ~1));   // [CELLS]
    __shared__ int spawn_count_s;
    const int tid = threadIdx.x;
    // chunks of EPB envs grid-stride, as step_shared_kernel: the set-up is paid once per workgroup and the next chunk's
    // per-env inputs are loaded while the current one is rendered
    const int64_t nchunks = (a.n + EPB - 1) / EPB;
    int64_t chunk = blockIdx.x;
    int64_t blockbase = chunk * EPB;
    int nb = (int)min((int64_t)EPB, a.n - blockbase);
    const bool masked = !DO_STEP && a.mask != nullptr;
    const bool autoreset = DO_STEP && a.auto_reset;
    const uint64_t epoch = step_epoch(a, autoreset);
    EnvState in{};
    if (tid < nb) in = load_env<VARIANT, DO_STEP>(a, blockbase + tid);
    // large batches: the first 256 workgroups touch every line of this step's per-env inputs once, as step_shared_kernel does
    // (the same block, written out in both kernels: see there)
    int warmed = 0;
    if (DO_STEP && (a.launch_hint & 0x100)) {
        warmed = warm_lines(a.action, a.n * 4, 256) + warm_lines(a.ball, a.n * 8, 256) + warm_lines(a.step_count, a.n * 4, 256);
        if (!V3) warmed += warm_lines(a.reward, a.n * 4, 256);
        if (V3) warmed += warm_lines(a.goal, a.n * 8, 256);
        if (autoreset) warmed += warm_lines(a.done, a.n, 256);
    }
    // set-up: ONE global round trip (the layout bytes, beside the env loads above), then everything from LDS
    for (int i = tid; i < CELLS; i += LMAZE_BLOCK) lay[i] = a.layout[i];
    __syncthreads();
    uint8_t* patb = reinterpret_cast<uint8_t*>(patw);
    for (int i = tid; i < 4 * PW; i += LMAZE_BLOCK) {                   // one dword of one copy per lane-iteration
        const int s = i / PW, k = (i - s * PW) << 2;                    // bytes k .. k+3 of copy s = pattern bytes k+s .. of the doubled row
        uint32_t w = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            int c = k + s + j;
            c -= c >= CELLS ? CELLS : 0;
            c -= c >= CELLS ? CELLS : 0;
            c = min(c, CELLS - 1);                                       // slack bytes past the doubled row: never selected
            w |= (uint32_t)cell_bits<VARIANT>(lay[c]) << (8 * j);
        }
        patw[i] = w;
    }
    if (autoreset && tid < 64) {
        const int cnt = wave_build_spawn_list<VARIANT>(lay, G, CELLS, spawn, tid);
        if (tid == 0) spawn_count_s = cnt;
    }
    if (tid == 0) { ballflat[EPB] = -64; goalflat[EPB] = -64; maskflag[EPB] = 0; }
    __syncthreads();
  for (;;) {
    const int64_t next = chunk + gridDim.x;
    const bool has_next = next < nchunks;                               // uniform over the workgroup
    EnvState in_next{};
    int nb_next = 0;
    if (has_next) {
        nb_next = (int)min((int64_t)EPB, a.n - next * EPB);
        if (tid < nb_next) in_next = load_env<VARIANT, DO_STEP>(a, next * EPB + tid);
    }
    if (tid < EPB) {
        int bf = -64, gf = -64, mf = 0;
        if (tid < nb) {
            const int64_t e = blockbase + tid;
            int bc, gc;
            const int cnt = autoreset ? spawn_count_s : 0;
            env_phase1<VARIANT, DO_STEP>(a, lay, G, e, in, [&](uint4 d, int& pb, int& pg) { place_from_list<VARIANT>(spawn, cnt, d, pb, pg); }, epoch, bc, gc);
            bf = bc;
            if (V3 && gc >= 0) gf = gc;
            if (masked) mf = a.mask[e] != 0;
        }
        ballflat[tid] = bf;
        goalflat[tid] = gf;
        maskflag[tid] = mf;
    }
    if (a.obs8 != nullptr) {
    __syncthreads();
    uint8_t* obs = a.obs8 + (size_t)blockbase * CELLS;
    const int R = nb * CELLS;
    if (!masked) {
        const int nq = R >> 4;
        for (int q = tid; q < nq; q += LMAZE_BLOCK) {
            const int f0 = q << 4;
            const int le = f0 / CELLS, c = f0 - le * CELLS;             // first cell of the store
            const int sft = c & 3;
            const uint32_t* src = patw + sft * PW + ((c - sft) >> 2);
            uint32_t w[4] = {src[0], src[1], src[2], src[3]};
            // ball (and v3 goal) bytes of env le at byte b - c, of env le + 1 at byte CELLS - c + b'
            const int b0 = ballflat[le] - c, b1 = CELLS - c + ballflat[min(le + 1, EPB)];
            if ((unsigned)b0 < 16u) w[b0 >> 2] |= (uint32_t)LMAZE_OBS_BALL << ((b0 & 3) << 3);
            if ((unsigned)b1 < 16u && le + 1 < nb) w[b1 >> 2] |= (uint32_t)LMAZE_OBS_BALL << ((b1 & 3) << 3);
            if (V3) {
                // gn < 0: env le + 1 has no goal on the grid.  Its -64 is no cell: added to CELLS - c it lands inside this
                // store wherever G*G >= 64, on cell G*G - 64 of env le (rollout_render_u8 asks the same)
                const int gn = goalflat[min(le + 1, EPB)];
                const int g0 = goalflat[le] - c, g1 = CELLS - c + gn;
                if ((unsigned)g0 < 16u) w[g0 >> 2] |= (uint32_t)LMAZE_OBS_GOAL << ((g0 & 3) << 3);
                if ((unsigned)g1 < 16u && gn >= 0 && le + 1 < nb) w[g1 >> 2] |= (uint32_t)LMAZE_OBS_GOAL << ((g1 & 3) << 3);
            }
            if (a.launch_hint & 0x100) {                                // set by the launcher for large batches: non-temporal stores
                typedef unsigned v4u __attribute__((ext_vector_type(4)));
                v4u t = {w[0], w[1], w[2], w[3]};
                stream_store16(reinterpret_cast<v4u*>(obs) + q, t);
            } else {
                reinterpret_cast<uint4*>(obs)[q] = make_uint4(w[0], w[1], w[2], w[3]);
            }
        }
        for (int f = (nq << 4) + tid; f < R; f += LMAZE_BLOCK) {        // ragged tail of the last chunk
            const int le = f / CELLS, c = f - le * CELLS;
            obs[f] = (uint8_t)(patb[c] | (ballflat[le] == c ? LMAZE_OBS_BALL : 0) | (V3 && goalflat[le] == c ? LMAZE_OBS_GOAL : 0));
        }
    } else {
        for (int f = tid; f < R; f += LMAZE_BLOCK) {                    // masked re-render (after a masked reset): byte stores
            const int le = f / CELLS, c = f - le * CELLS;
            if (!maskflag[le]) continue;
            obs[f] = (uint8_t)(patb[c] | (ballflat[le] == c ? LMAZE_OBS_BALL : 0) | (V3 && goalflat[le] == c ? LMAZE_OBS_GOAL : 0));
        }
    }
    }
    if (!has_next) break;
    __syncthreads();                                                     // the per-env cells in LDS are rewritten by the next chunk
    chunk = next;
    blockbase = chunk * EPB;
    nb = nb_next;
    in = in_next;
  }
    if (warmed == 0x7fedcba9 && a.n < 0) a.done[0] = 1;   // never true: keeps the warming loads alive
}

// ------------------------------------------------------------------------------------
// T steps in ONE launch for the same on-die 8x8 batches (lmaze_rollout_v0 / _v3): the wave-autonomous kernel above with
// the step loop inside.  A wave's 64 envs stay in registers for the whole rollout -- envs are independent, nothing
// synchronises --, each step's action row is fetched one step ahead, the planes are rewritten every step exactly as T
// launches would (same 16 KiB per wave: they stay in L2) and the per-env state goes back once at the end; optional
// per-step reward / done rows for the caller who needs the trajectory.  Step t draws its placements with epoch + t, as
// the t-th of T lmaze_step_*_autoreset calls would.  Bit-identical to those T calls.
// ------------------------------------------------------------------------------------
struct RolloutArgs {
    const int32_t* actions;   // [T, N]
    float* reward_t;          // [T, N] or null
    uint8_t* done_t;          // [T, N] or null
    int32_t T;
};

// The recording rollout (lmaze_rollout_obs): the kernels below take this type instead of RolloutArgs -- an overload of
// each kernel, so the plain forms keep their symbols and code.  Step t stores its planes into slot j of obs_t when
// t = (j + 1) every - 1, into the caller's obs when it is the last step, and nowhere otherwise: the destination of a step
// is uniform over the workgroup (wave), and a step that records nothing skips its render and its barriers.
struct RolloutObsArgs : RolloutArgs {
    int32_t* obs_t;           // [T / every, N, G, G] or null (every == 0: final planes only)
    int32_t every;            // k >= 1, or 0
    int32_t nt;               // slot stores: non-temporal (1) or plain (0), chosen by the launcher
};

// The slot step t of the recording form fills -- slot j when t = (j + 1) every - 1 -- at this workgroup's (wave's) first
// env `base`, or null.  Uniform: one scalar division per step.
__device__ __forceinline__ int32_t* rollout_slot(const RolloutObsArgs& ro, int64_t n, int64_t base, int cells, int t) {
    if (ro.obs_t == nullptr || ro.every <= 0 || (t + 1) % ro.every != 0) return nullptr;
    return ro.obs_t + ((size_t)((t + 1) / ro.every - 1) * n + base) * cells;
}
__device__ __forceinline__ int32_t* rollout_slot(const RolloutArgs&, int64_t, int64_t, int, int) { return nullptr; }
__device__ __forceinline__ bool slot_nt(const RolloutArgs&) { return false; }
__device__ __forceinline__ bool slot_nt(const RolloutObsArgs& ro) { return ro.nt != 0; }

// The rollout kernels' registers, loaded once: the env's state with the action row of step 0 in act (a lane without
// an env holds a neutral one)
template <int VARIANT>
__device__ __forceinline__ EnvState rollout_load(const StepArgs& a, const RolloutArgs& ro, int64_t e, bool live) {
    EnvState s;
    s.b = make_int2(1, 1); s.g = make_int2(-1, -1);
    s.act = -1; s.sc = 0; s.done = 0; s.r = 0.0f;
    if (live) {
        s.b = a.ball[e];
        if (VARIANT == LMAZE_VARIANT_V3) s.g = a.goal[e];
        s.sc = a.step_count[e];
        if (VARIANT != LMAZE_VARIANT_V3) s.r = a.reward[e];
        if (a.auto_reset) s.done = a.done[e];
        s.act = ro.actions[e];
    }
    return s;
}

// step t's reward / done rows, for the caller who asked for the trajectory
__device__ __forceinline__ void rollout_record(const RolloutArgs& ro, int64_t n, int t, int64_t e, const EnvState& s) {
    if (ro.reward_t) ro.reward_t[(size_t)t * n + e] = s.r;
    if (ro.done_t) ro.done_t[(size_t)t * n + e] = s.done;
}

// the state goes back once, at the end of the rollout: v3's goal only when the fused reset can have moved it
template <int VARIANT>
__device__ __forceinline__ void rollout_store(const StepArgs& a, const RolloutArgs& ro, int64_t e, bool live, const EnvState& s,
                                              int hits) {
    if (live && ro.T > 0) {
        a.ball[e] = s.b;
        if (VARIANT == LMAZE_VARIANT_V3 && a.auto_reset) a.goal_rw[e] = s.g;
        a.step_count[e] = s.sc;
        a.reward[e] = s.r;
        a.done[e] = s.done;
        if (hits && a.goal_count) a.goal_count[e] += hits;
    }
}


template <int VARIANT, int EPW>
__global__ __launch_bounds__(LMAZE_BLOCK) void rollout_shared_wave8_kernel(const StepArgs a, const RolloutArgs ro) {
    constexpr bool REC = false;
#define LMAZE_ROLLOUT_BODY 1
#include "lmaze_rollout_body.h"
#undef LMAZE_ROLLOUT_BODY
}

// the recording form (lmaze_rollout_obs)
template <int VARIANT, int EPW>
__global__ __launch_bounds__(LMAZE_BLOCK) __attribute__((amdgpu_waves_per_eu(6))) void rollout_shared_wave8_kernel(const StepArgs a, const RolloutObsArgs ro) {
    constexpr bool REC = true;
#define LMAZE_ROLLOUT_BODY 1
#include "lmaze_rollout_body.h"
#undef LMAZE_ROLLOUT_BODY
}

// One step's planes of a rollout workgroup (R dwords): dword f of the range = cell f % CELLS of env f / CELLS, a lane
// walking its 16-byte stores 1024 dwords apart, then the ragged tail (nb*G*G not a multiple of 4).  bits(le, c) = the
// ball-free plane bits of cell c of env le.  nt: non-temporal 16-byte stores (the recording form's slots).
template <int VARIANT, class Bits>
__device__ __forceinline__ void rollout_render(int32_t* obs, int R, int CELLS, const int* ballflat, const int* goalflat, Bits bits,
                                               bool nt = false) {
    const int tid = threadIdx.x, nq = R >> 2;
    auto value = [&](int le, int c) {
        int v = bits(le, c);
        v |= (ballflat[le] == c) ? LMAZE_OBS_BALL : 0;
        if (VARIANT == LMAZE_VARIANT_V3) v |= (goalflat[le] == c) ? LMAZE_OBS_GOAL : 0;
        return v;
    };
    int le = (tid << 2) / CELLS, c = (tid << 2) - le * CELLS;
    const int dle = (LMAZE_BLOCK << 2) / CELLS, dc = (LMAZE_BLOCK << 2) - dle * CELLS;
    for (int q = tid; q < nq; q += LMAZE_BLOCK) {
        int vals[4], l2 = le, c2 = c;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            vals[j] = value(l2, c2);
            if (++c2 == CELLS) { c2 = 0; ++l2; }
        }
        if (nt) store16<true>(reinterpret_cast<int4*>(obs) + q, make_int4(vals[0], vals[1], vals[2], vals[3]));
        else reinterpret_cast<int4*>(obs)[q] = make_int4(vals[0], vals[1], vals[2], vals[3]);
        le += dle; c += dc;
        if (c >= CELLS) { c -= CELLS; ++le; }
    }
    const int f = (nq << 2) + tid;
    if (f < R) {
        const int l2 = f / CELLS;
        obs[f] = value(l2, f - l2 * CELLS);
    }
}

// T steps of a shared-layout batch of ANY grid size in one launch, for batches whose planes stay on-die: a workgroup owns
// EPB envs for the whole rollout -- one lane per env keeps ball, goal, stepCount, reward and done in registers across the
// T steps, the layout, its plane pattern and the spawn list are set up in LDS once -- and re-renders its envs' planes after
// every step exactly as T launches of step_shared_kernel would (two barriers per step, no grid-wide one: envs are
// independent).  Per-step launches of such a batch are launch-bound (65 536 x 11x11: 8 us per launch for 32 MB of planes
// that never leave the caches).  Transition, fused reset (placement from the compacted spawn list with the draw of
// epoch + t) and the v0 reward persistence are the step kernel's own functions: bit-identical by construction and by test.

template <int VARIANT>
__global__ __launch_bounds__(LMAZE_BLOCK) void rollout_shared_kernel(const StepArgs a, const RolloutArgs ro) {
    constexpr bool REC = false;
#define LMAZE_ROLLOUT_BODY 2
#include "lmaze_rollout_body.h"
#undef LMAZE_ROLLOUT_BODY
}

// the recording form (lmaze_rollout_obs)
template <int VARIANT>
__global__ __launch_bounds__(LMAZE_BLOCK) __attribute__((amdgpu_waves_per_eu(8))) void rollout_shared_kernel(const StepArgs a, const RolloutObsArgs ro) {
    constexpr bool REC = true;
#define LMAZE_ROLLOUT_BODY 2
#include "lmaze_rollout_body.h"
#undef LMAZE_ROLLOUT_BODY
}

// The same for per-env layouts: the workgroup's EPB layouts (EPB * G * G bytes) are copied to LDS once and serve the
// collision check, the planes and -- a done env, fused reset -- the whole-wave placement on the env's own maze (wave_place,
// the rule of the per-env step kernels) for all T steps.  EPB <= 64: every env's lane sits in wave 0, which places the
// done envs one after the other.

template <int VARIANT>
__global__ __launch_bounds__(LMAZE_BLOCK) void rollout_perenv_kernel(const StepArgs a, const RolloutArgs ro) {
    constexpr bool REC = false;
#define LMAZE_ROLLOUT_BODY 3
#include "lmaze_rollout_body.h"
#undef LMAZE_ROLLOUT_BODY
}

// the recording form (lmaze_rollout_obs)
template <int VARIANT>
__global__ __launch_bounds__(LMAZE_BLOCK) __attribute__((amdgpu_waves_per_eu(7))) void rollout_perenv_kernel(const StepArgs a, const RolloutObsArgs ro) {
    constexpr bool REC = true;
#define LMAZE_ROLLOUT_BODY 3
#include "lmaze_rollout_body.h"
#undef LMAZE_ROLLOUT_BODY
}

// ------------------------------------------------------------------------------------
// T steps of a shared-layout batch with the NARROW planes (lmaze_rollout_u8 / lmaze_rollout_obs_u8): rollout_shared_kernel's
// workgroup -- EPB envs for all T steps, one lane per env with its state in registers -- set up as step_shared_u8_kernel
// (layout, byte-shifted pattern copies, spawn list in LDS once) and rendering as it does, 16 cells per 16-byte store.
// ------------------------------------------------------------------------------------

// The recording form of the u8 rollout: RolloutObsArgs with uint8 slots (a type of its own, so that the int32 recording
// kernels keep theirs).  Slot j = obs_t8 + j N G G bytes: past slot 0 it starts wherever N G G puts it.
struct RolloutObs8Args : RolloutArgs {
    uint8_t* obs_t8;          // [T / every, N, G, G] or null (every == 0: final planes only)
    int32_t every;            // k >= 1, or 0
};

__device__ __forceinline__ uint8_t* rollout_slot8(const RolloutObs8Args& ro, int64_t n, int64_t base, int cells, int t) {
    if (ro.obs_t8 == nullptr || ro.every <= 0 || (t + 1) % ro.every != 0) return nullptr;
    return ro.obs_t8 + ((size_t)((t + 1) / ro.every - 1) * n + base) * cells;
}
__device__ __forceinline__ uint8_t* rollout_slot8(const RolloutArgs&, int64_t, int64_t, int, int) { return nullptr; }

// One step's narrow planes of a u8 rollout workgroup: R = nb G*G bytes at dst, byte f = cell f % CELLS of env f / CELLS.
// dst is 16-byte aligned for obs8 and slot 0, but slot j > 0 starts j N G G bytes past a 16-byte boundary (N = 777 at
// 11x11: 5 bytes past one), so no store may assume it.  The range is cut at absolute 16-byte boundaries:
//   head  bytes [0, h) up to the first boundary at or after dst (h < 16): byte stores
//   body  the whole aligned granules inside the range: one 16-byte store of 16 cells each, as step_shared_u8_kernel's
//   tail  the bytes after the last whole granule (< 16): byte stores
// Why nothing is written twice or outside the range: every 16-byte store covers one aligned granule that lies wholly
// inside [dst, dst + R); a granule that the range shares with a neighbour -- the next workgroup's range or the next slot,
// or what lies before and after obs_t8 -- is only ever written here by byte stores to this range's own bytes, and the
// neighbour writes its own bytes of it the same way.  A byte store is a byte-masked write, not a read-modify-write, so
// the two sides of a shared granule never overwrite each other, whatever order they land in.
template <int VARIANT>
__device__ __forceinline__ void rollout_render_u8(uint8_t* dst, int R, int CELLS, int nb, const uint32_t* patw, int PW,
                                                  const int* ballflat, const int* goalflat) {
    constexpr bool V3 = VARIANT == LMAZE_VARIANT_V3;
    const int tid = threadIdx.x;
    const int h = min((int)((16u - ((unsigned)(uintptr_t)dst & 15u)) & 15u), R);
    const int nq = (R - h) >> 4;
    uint4* dst4 = reinterpret_cast<uint4*>(dst + h);
    for (int q = tid; q < nq; q += LMAZE_BLOCK) {
        const int f0 = h + (q << 4);
        const int le = f0 / CELLS, c = f0 - le * CELLS;                 // first cell of the store; G >= 4: at most two envs
        const int sft = c & 3;
        const uint32_t* src = patw + sft * PW + ((c - sft) >> 2);
        uint32_t w[4] = {src[0], src[1], src[2], src[3]};
        const int b0 = ballflat[le] - c;
        if ((unsigned)b0 < 16u) w[b0 >> 2] |= (uint32_t)LMAZE_OBS_BALL << ((b0 & 3) << 3);
        if (V3) {
            const int g0 = goalflat[le] - c;
            if ((unsigned)g0 < 16u) w[g0 >> 2] |= (uint32_t)LMAZE_OBS_GOAL << ((g0 & 3) << 3);
        }
        if (c > CELLS - 16 && le + 1 < nb) {                             // the store runs into env le + 1 at byte CELLS - c
            const int b1 = CELLS - c + ballflat[le + 1];
            if ((unsigned)b1 < 16u) w[b1 >> 2] |= (uint32_t)LMAZE_OBS_BALL << ((b1 & 3) << 3);
            if (V3 && goalflat[le + 1] >= 0) {                           // < 0: no goal on the grid
                const int g1 = CELLS - c + goalflat[le + 1];
                if ((unsigned)g1 < 16u) w[g1 >> 2] |= (uint32_t)LMAZE_OBS_GOAL << ((g1 & 3) << 3);
            }
        }
        dst4[q] = make_uint4(w[0], w[1], w[2], w[3]);
    }
    const int t0 = h + (nq << 4);                                        // first byte of the tail
    if (tid < h + (R - t0)) {                                            // head and tail: at most 30 bytes
        const int f = tid < h ? tid : t0 + (tid - h);
        const int le = f / CELLS, c = f - le * CELLS;
        const uint8_t* patb = reinterpret_cast<const uint8_t*>(patw);   // copy 0: pattern byte c
        dst[f] = (uint8_t)(patb[c] | (ballflat[le] == c ? LMAZE_OBS_BALL : 0) | (V3 && goalflat[le] == c ? LMAZE_OBS_GOAL : 0));
    }
}

template <int VARIANT>
__global__ __launch_bounds__(LMAZE_BLOCK) void rollout_shared_u8_kernel(const StepArgs a, const RolloutArgs ro) {
    constexpr bool REC = false;
#define LMAZE_ROLLOUT_BODY 4
#include "lmaze_rollout_body.h"
#undef LMAZE_ROLLOUT_BODY
}

// the recording form (lmaze_rollout_obs_u8)
template <int VARIANT>
__global__ __launch_bounds__(LMAZE_BLOCK) void rollout_shared_u8_kernel(const StepArgs a, const RolloutObs8Args ro) {
    constexpr bool REC = true;
#define LMAZE_ROLLOUT_BODY 4
#include "lmaze_rollout_body.h"
#undef LMAZE_ROLLOUT_BODY
}

// ------------------------------------------------------------------------------------
// Closed-loop rollouts (lmaze_rollout_policy / lmaze_rollout_policy_u8): the three workgroup kernels above with a tabular
// epsilon-greedy policy in place of the action row.  A table policy needs no planes -- the key is the ball's cell and, goal-
// conditioned (v3), the goal's, both in the owning lane's registers -- so the rollout stays ONE launch: per env-step one
// table lookup (ball-keyed: G*G bytes staged in LDS once per workgroup; goal-conditioned: G^4 bytes read from global
// memory, L2-resident) and, when exploring, one Philox draw.  New overloads on new argument types, as the recording forms
// were added: the open-loop kernels keep their symbols and code.  Recording semantics only (REC): planes are stored on
// recorded steps and after the last one.
// ------------------------------------------------------------------------------------
// PolicyTable: lmaze_common.h
struct RolloutPolicyArgs : RolloutObsArgs { PolicyTable pol; };     // actions: null, never read
struct RolloutPolicy8Args : RolloutObs8Args { PolicyTable pol; };

// rollout_load without an action row
template <int VARIANT>
__device__ __forceinline__ EnvState policy_load(const StepArgs& a, int64_t e, bool live) {
    EnvState s;
    s.b = make_int2(1, 1); s.g = make_int2(-1, -1);
    s.act = -1; s.sc = 0; s.done = 0; s.r = 0.0f;
    if (live) {
        s.b = a.ball[e];
        if (VARIANT == LMAZE_VARIANT_V3) s.g = a.goal[e];
        s.sc = a.step_count[e];
        if (VARIANT != LMAZE_VARIANT_V3) s.r = a.reward[e];
        if (a.auto_reset) s.done = a.done[e];
    }
    return s;
}

// Step t's action of env e (workgroup-local state s, after the fused reset): key -> table -> epsilon mix, and the rows of
// the caller who asked for them.  Coordinates enter the key as the transition takes them, clamped onto the grid, so a
// lookup never leaves the table.  tab: the ball-keyed table in LDS.
template <int VARIANT>
__device__ __forceinline__ void policy_act(const StepArgs& a, const PolicyTable& p, const uint8_t* tab, int G, int t, int64_t e,
                                           EnvState& s) {
    int key = clampi(s.b.x, 0, G - 1) * G + clampi(s.b.y, 0, G - 1);
    int act;
    if (VARIANT == LMAZE_VARIANT_V3 && p.key_mode != 0) {
        key += (clampi(s.g.x, 0, G - 1) * G + clampi(s.g.y, 0, G - 1)) * G * G;
        act = p.table[key];
    } else {
        act = tab[key];
    }
    if (p.epsilon != 0) {                                             // uniform
        const uint4 r = policy_draw(a.seed, a.epoch + (uint64_t)t, a.env_base + e);
        if (r.x < p.epsilon) act = (int)(r.y >> 30);
    }
    s.act = act;
    if (p.actions_t) p.actions_t[(size_t)t * a.n + e] = act;
    if (p.key_t) p.key_t[(size_t)t * a.n + e] = key;
}

#define LMAZE_ROLLOUT_POLICY 1
template <int VARIANT>
__global__ __launch_bounds__(LMAZE_BLOCK) __attribute__((amdgpu_waves_per_eu(8))) void rollout_shared_kernel(const StepArgs a, const RolloutPolicyArgs ro) {
    constexpr bool REC = true;
#define LMAZE_ROLLOUT_BODY 2
#include "lmaze_rollout_body.h"
#undef LMAZE_ROLLOUT_BODY
}

template <int VARIANT>
__global__ __launch_bounds__(LMAZE_BLOCK) __attribute__((amdgpu_waves_per_eu(7))) void rollout_perenv_kernel(const StepArgs a, const RolloutPolicyArgs ro) {
    constexpr bool REC = true;
#define LMAZE_ROLLOUT_BODY 3
#include "lmaze_rollout_body.h"
#undef LMAZE_ROLLOUT_BODY
}

// no occupancy target: at 6 waves per SIMD (the v0 recording twin's) the v0 form spills 12 bytes per lane; as it is, 91 (v0) /
// 88 (v3) VGPRs, 5 waves.
// CLOSED is always true and selects nothing.  It is here for the symbol only: tests/test_rollout_u8_cpu.py lists every
// instantiation named rollout_shared_u8_kernel<VARIANT> (one template argument) and requires exactly the four open-loop
// ones; with a second argument the closed-loop form is still an overload of the same kernel but not one of those names.
template <int VARIANT, bool CLOSED>
__global__ __launch_bounds__(LMAZE_BLOCK) void rollout_shared_u8_kernel(const StepArgs a, const RolloutPolicy8Args ro) {
    constexpr bool REC = true;
#define LMAZE_ROLLOUT_BODY 4
#include "lmaze_rollout_body.h"
#undef LMAZE_ROLLOUT_BODY
}
#undef LMAZE_ROLLOUT_POLICY

// ------------------------------------------------------------------------------------
// Sampling closed-loop rollouts (lmaze_rollout_sample / lmaze_rollout_sample_u8): the closed-loop forms above with a
// categorical table policy -- per key one uint4 (c0, c1, c2, reserved) of cumulative thresholds, and per env-step one
// Philox draw r = policy_draw(...).x compared against them: action = (r >= c0) + (r >= c1) + (r >= c2) (include/lmaze.h).
// The ball-keyed table of G <= 32 (at most 16 KiB) is staged in LDS once per workgroup with 16-byte copies and read with
// one 128-bit LDS read per env-step; every other table (goal-conditioned, or G > 32) is read from global memory, one
// 16-byte read per env-step, L2- or Infinity-Cache-resident.  The host decides (rollout_plan) and passes `staged`.
// Again new overloads on new argument types, bodies 2-4 with LMAZE_ROLLOUT_POLICY == 2.
// ------------------------------------------------------------------------------------
// sample_row_t, SampleTable: lmaze_common.h
struct RolloutSampleArgs : RolloutObsArgs { SampleTable pol; };     // actions: null, never read
struct RolloutSample8Args : RolloutObs8Args { SampleTable pol; };

// Step t's action of env e (workgroup-local state s, after the fused reset): key -> thresholds -> three unsigned compares
// of the draw, and the rows of the caller who asked for them.  The key is policy_act's: clamped onto the grid.  tab: the
// staged table in LDS.  Nothing is validated: any row yields an action in 0..3.
// The two reads go through pointers of their own address spaces: as two generic loads the compiler merged them into one
// flat load of a selected pointer, which waits on both counters and is neither an LDS read nor a global one.  The row is
// read whole -- word 3 is kept alive to the end -- so it is one 128-bit read on either path, issued before the draw.
template <int VARIANT>
__device__ __forceinline__ void policy_act(const StepArgs& a, const SampleTable& p, const sample_row_t* tab, int G, int t, int64_t e,
                                           EnvState& s) {
    typedef const __attribute__((address_space(3))) sample_row_t* lds_rows;
    typedef const __attribute__((address_space(1))) sample_row_t* global_rows;
    int key = clampi(s.b.x, 0, G - 1) * G + clampi(s.b.y, 0, G - 1);
    sample_row_t c;
    if (VARIANT == LMAZE_VARIANT_V3 && p.key_mode != 0) {
        key += (clampi(s.g.x, 0, G - 1) * G + clampi(s.g.y, 0, G - 1)) * G * G;
        c = ((global_rows)p.table)[key];
    } else if (p.staged) {
        c = ((lds_rows)tab)[key];
    } else {
        c = ((global_rows)p.table)[key];
    }
    const uint32_t r = policy_draw(a.seed, a.epoch + (uint64_t)t, a.env_base + e).x;
    const int act = (int)(r >= c.x) + (int)(r >= c.y) + (int)(r >= c.z);
    asm volatile("" ::"v"(c.w));
    s.act = act;
    if (p.actions_t) p.actions_t[(size_t)t * a.n + e] = act;
    if (p.key_t) p.key_t[(size_t)t * a.n + e] = key;
}

#define LMAZE_ROLLOUT_POLICY 2
template <int VARIANT>
__global__ __launch_bounds__(LMAZE_BLOCK) __attribute__((amdgpu_waves_per_eu(8))) void rollout_shared_kernel(const StepArgs a, const RolloutSampleArgs ro) {
    constexpr bool REC = true;
#define LMAZE_ROLLOUT_BODY 2
#include "lmaze_rollout_body.h"
#undef LMAZE_ROLLOUT_BODY
}

template <int VARIANT>
__global__ __launch_bounds__(LMAZE_BLOCK) __attribute__((amdgpu_waves_per_eu(7))) void rollout_perenv_kernel(const StepArgs a, const RolloutSampleArgs ro) {
    constexpr bool REC = true;
#define LMAZE_ROLLOUT_BODY 3
#include "lmaze_rollout_body.h"
#undef LMAZE_ROLLOUT_BODY
}

// CLOSED as in the epsilon-greedy form: for the symbol only
template <int VARIANT, bool CLOSED>
__global__ __launch_bounds__(LMAZE_BLOCK) void rollout_shared_u8_kernel(const StepArgs a, const RolloutSample8Args ro) {
    constexpr bool REC = true;
#define LMAZE_ROLLOUT_BODY 4
#include "lmaze_rollout_body.h"
#undef LMAZE_ROLLOUT_BODY
}
#undef LMAZE_ROLLOUT_POLICY

// ------------------------------------------------------------------------------------
// Closed-loop rollouts with a table PER ENV (lmaze_env_rollout_policy / lmaze_env_rollout_sample): what lmaze_solve returns for
// per-env layouts, or a population of policies on one shared maze.  The forms above with one more key rule -- row
// i * G^2 + ball cell of env i, the workgroup-local index blockbase + tid and not env_base + i -- and everything else theirs:
// the fused reset, the draw, the compares, the rows, the planes.  Again new overloads on new argument types, bodies 2 and 3
// with LMAZE_ROLLOUT_POLICY == 3 (epsilon-greedy) and 4 (sampling); int32 planes only.
// Where the table is read.  rollout_perenv_kernel, epsilon-greedy: the workgroup's EPB * G^2 table bytes are staged into LDS
// once, behind its layouts and by the same dword copy -- the lookup sits on the dependent chain of every env-step (state ->
// key -> action -> transition -> state), a dependent LDS read costs a quarter of an L2 hit, and the rows are read T times.
// Sampling (16 bytes per cell and env do not fit beside the layouts) and both forms of rollout_shared_kernel: from global
// memory, the env's own rows, one byte or one 128-bit read per env-step.
// ------------------------------------------------------------------------------------
// EnvPolicyTable, EnvSampleTable: lmaze_common.h
struct RolloutEnvBytesArgs : RolloutObsArgs { EnvPolicyTable pol; };   // actions: null, never read
struct RolloutEnvRowsArgs : RolloutObsArgs { EnvSampleTable pol; };

// The lane's table pointers carry their address space, for the reason given above policy_act(SampleTable): a generic load
// is neither an LDS read nor a global one.
typedef const __attribute__((address_space(3))) uint8_t* env_bytes_lds;
typedef const __attribute__((address_space(1))) uint8_t* env_bytes_global;
typedef const __attribute__((address_space(1))) sample_row_t* env_rows_global;
__device__ __forceinline__ env_bytes_global env_table_global(const EnvPolicyTable& p) { return (env_bytes_global)p.table; }
__device__ __forceinline__ env_rows_global env_table_global(const EnvSampleTable& p) { return (env_rows_global)p.table; }

// policy_act(PolicyTable) with the env's own table: row = its G^2 bytes (in LDS or in global memory), e the local index
template <int VARIANT, class Row>
__device__ __forceinline__ void policy_act(const StepArgs& a, const EnvPolicyTable& p, Row row, int G, int t, int64_t e, EnvState& s) {
    const int cell = clampi(s.b.x, 0, G - 1) * G + clampi(s.b.y, 0, G - 1);
    int act = row[cell];
    if (p.epsilon != 0) {                                             // uniform
        const uint4 r = policy_draw(a.seed, a.epoch + (uint64_t)t, a.env_base + e);
        if (r.x < p.epsilon) act = (int)(r.y >> 30);
    }
    s.act = act;
    if (p.actions_t) p.actions_t[(size_t)t * a.n + e] = act;
    if (p.key_t) p.key_t[(size_t)t * a.n + e] = (int)e * G * G + cell;
}

// policy_act(SampleTable) with the env's own rows in global memory: one 128-bit read, issued before the draw
template <int VARIANT>
__device__ __forceinline__ void policy_act(const StepArgs& a, const EnvSampleTable& p, env_rows_global row, int G, int t, int64_t e,
                                           EnvState& s) {
    const int cell = clampi(s.b.x, 0, G - 1) * G + clampi(s.b.y, 0, G - 1);
    const sample_row_t c = row[cell];
    const uint32_t r = policy_draw(a.seed, a.epoch + (uint64_t)t, a.env_base + e).x;
    const int act = (int)(r >= c.x) + (int)(r >= c.y) + (int)(r >= c.z);
    asm volatile("" ::"v"(c.w));
    s.act = act;
    if (p.actions_t) p.actions_t[(size_t)t * a.n + e] = act;
    if (p.key_t) p.key_t[(size_t)t * a.n + e] = (int)e * G * G + cell;
}

#define LMAZE_ROLLOUT_POLICY 3
template <int VARIANT>
__global__ __launch_bounds__(LMAZE_BLOCK) __attribute__((amdgpu_waves_per_eu(8))) void rollout_shared_kernel(const StepArgs a, const RolloutEnvBytesArgs ro) {
    constexpr bool REC = true;
#define LMAZE_ROLLOUT_BODY 2
#include "lmaze_rollout_body.h"
#undef LMAZE_ROLLOUT_BODY
}

template <int VARIANT>
__global__ __launch_bounds__(LMAZE_BLOCK) __attribute__((amdgpu_waves_per_eu(7))) void rollout_perenv_kernel(const StepArgs a, const RolloutEnvBytesArgs ro) {
    constexpr bool REC = true;
#define LMAZE_ROLLOUT_BODY 3
#include "lmaze_rollout_body.h"
#undef LMAZE_ROLLOUT_BODY
}
#undef LMAZE_ROLLOUT_POLICY

#define LMAZE_ROLLOUT_POLICY 4
template <int VARIANT>
__global__ __launch_bounds__(LMAZE_BLOCK) __attribute__((amdgpu_waves_per_eu(8))) void rollout_shared_kernel(const StepArgs a, const RolloutEnvRowsArgs ro) {
    constexpr bool REC = true;
#define LMAZE_ROLLOUT_BODY 2
#include "lmaze_rollout_body.h"
#undef LMAZE_ROLLOUT_BODY
}

template <int VARIANT>
__global__ __launch_bounds__(LMAZE_BLOCK) __attribute__((amdgpu_waves_per_eu(7))) void rollout_perenv_kernel(const StepArgs a, const RolloutEnvRowsArgs ro) {
    constexpr bool REC = true;
#define LMAZE_ROLLOUT_BODY 3
#include "lmaze_rollout_body.h"
#undef LMAZE_ROLLOUT_BODY
}
#undef LMAZE_ROLLOUT_POLICY

// ------------------------------------------------------------------------------------
// Q-learning inside the rollout (lmaze_env_rollout_qlearn): the forms with a table per env, where the table is float32 action
// values that the lane acts on epsilon-greedily AND updates after every transition -- N independent tabular learners, acting,
// stepping and learning T steps in ONE launch.  The lane that steps env i is the only reader and writer of table i, so an
// env's updates are a sequential float32 recurrence (lmaze_learn.h: lmaze_q_first_max, lmaze_q_target, lmaze_q_update, no
// fma) that a host loop reproduces bit for bit; a shared table would need atomics and an arbitrary update order.
// Per env-step: the row of the cell c the env stands on, after the transition the row of the cell c' it reached (128 bits,
// read BEFORE the write: the target bootstraps from the table as it stood), and the row of c written back whole with word a
// replaced.  Every access goes through one pointer type, q_rows_global -- address space 1, neither const nor __restrict__
// -- so no read of a later step can move above an earlier step's write of the same row (c' == c on every wall bump, and a
// ball that walks back reads what it wrote two steps before).
// The row of c' IS the row of c at step t + 1 unless a reset moves the ball, so the lane keeps it in registers (QLane::next_*,
// on a bump the row it has just written) and reads the table only where the cells differ: one dependent global round trip
// per env-step instead of two.  Measured against the build that reads both rows (tools/bench_qlearn.py, T = 64, us per step,
// medians of 9 rounds, two processes each, alternating): 16 384 x 11x11 per-env 1.86 against 1.99, 65 536 x 11x11 per-env
// 3.46 against 3.55, 16 384 x 32x32 per-env 3.63 against 3.72, 65 536 x 11x11 shared 2.64 against 2.76.  The five more
// registers do not fit the siblings' occupancy targets without 12 bytes of scratch per lane: 7 waves per SIMD asked for the
// shared-layout kernel (67 / 72 VGPRs, v0 / v3) and 6 for the per-env one (72 / 77); the figures above are at these.
// Bodies 2 and 3 with LMAZE_ROLLOUT_POLICY == 5; the table stays in global memory (LMAZE_TAB_GLOBAL: 16 bytes per cell and env
// do not fit LDS beside the layouts), int32 planes only.
// ------------------------------------------------------------------------------------
// EnvQTable, q_row_t: lmaze_common.h
struct RolloutEnvQArgs : RolloutObsArgs { EnvQTable pol; };           // actions: null, never read

typedef __attribute__((address_space(1))) q_row_t* q_rows_global;
__device__ __forceinline__ q_rows_global env_table_global(const EnvQTable& p) { return (q_rows_global)p.q; }
// What the owning lane carries: its env's rows; from the lookup to the update the cell it acted from and that cell's row;
// from the update to the next lookup the cell it reached and that cell's row
struct QLane {
    q_rows_global rows;
    int cell;
    q_row_t row;
    int next_cell;            // the cell the last transition reached (-1: none yet) and its row as the table now holds it
    q_row_t next_row;
};

// policy_act(EnvPolicyTable) with the greedy action taken from the env's own row of values: the first maximum
template <int VARIANT>
__device__ __forceinline__ void policy_act(const StepArgs& a, const EnvQTable& p, QLane& q, int G, int t, int64_t e, EnvState& s) {
    q.cell = clampi(s.b.x, 0, G - 1) * G + clampi(s.b.y, 0, G - 1);
    if (q.cell == q.next_cell) q.row = q.next_row;                    // carried: the same words the table holds
    else q.row = q.rows[q.cell];                                      // the first step, or a reset moved the ball
    const float v[4] = {q.row.x, q.row.y, q.row.z, q.row.w};
    int act;
    (void)lmaze_q_first_max(v, &act);
    if (p.epsilon != 0) {                                             // uniform
        const uint4 r = policy_draw(a.seed, a.epoch + (uint64_t)t, a.env_base + e);
        if (r.x < p.epsilon) act = (int)(r.y >> 30);
    }
    s.act = act;
    if (p.actions_t) p.actions_t[(size_t)t * a.n + e] = act;
    if (p.key_t) p.key_t[(size_t)t * a.n + e] = (int)e * G * G + q.cell;
}

// The update of the transition env_advance just made: s holds the cell reached, the step's reward and its own done flag
// (the step limit counts).  The word is chosen by compares, not by an index into the row: no scratch.
__device__ __forceinline__ void qlearn_update(const EnvQTable& p, QLane& q, int G, int64_t n, int t, int64_t e, const EnvState& s) {
    const q_row_t next = q.rows[ball_cell_of(s.b, G)];                // as the table stands before this step's write
    const float v[4] = {next.x, next.y, next.z, next.w};
    int greedy;
    const float v_next = lmaze_q_first_max(v, &greedy);
    const int act = s.act;
    const float q_sa = act == 0 ? q.row.x : act == 1 ? q.row.y : act == 2 ? q.row.z : q.row.w;
    float delta;
    const float q_new = lmaze_q_update(q_sa, p.alpha, lmaze_q_target(s.r, s.done, p.gamma, v_next), &delta);
    q_row_t w = q.row;
    w.x = act == 0 ? q_new : w.x;
    w.y = act == 1 ? q_new : w.y;
    w.z = act == 2 ? q_new : w.z;
    w.w = act == 3 ? q_new : w.w;
    q.rows[q.cell] = w;
    q.next_cell = ball_cell_of(s.b, G);
    q.next_row = q.next_cell == q.cell ? w : next;                    // a bump: the row just written
    if (p.td_t) p.td_t[(size_t)t * n + e] = delta;
}

#define LMAZE_ROLLOUT_POLICY 5
template <int VARIANT>
__global__ __launch_bounds__(LMAZE_BLOCK) __attribute__((amdgpu_waves_per_eu(7))) void rollout_shared_kernel(const StepArgs a, const RolloutEnvQArgs ro) {
    constexpr bool REC = true;
#define LMAZE_ROLLOUT_BODY 2
#include "lmaze_rollout_body.h"
#undef LMAZE_ROLLOUT_BODY
}

template <int VARIANT>
__global__ __launch_bounds__(LMAZE_BLOCK) __attribute__((amdgpu_waves_per_eu(6))) void rollout_perenv_kernel(const StepArgs a, const RolloutEnvQArgs ro) {
    constexpr bool REC = true;
#define LMAZE_ROLLOUT_BODY 3
#include "lmaze_rollout_body.h"
#undef LMAZE_ROLLOUT_BODY
}
#undef LMAZE_ROLLOUT_POLICY

// ------------------------------------------------------------------------------------
// host launchers
// ------------------------------------------------------------------------------------

static size_t shared_lds_bytes(int G, bool specialised, int epb, bool with_marks) {
    const int cells = G * G;
    const int pat = (specialised && (G & 1)) ? 4 * cells : cells;
    // pattern + ballflat/goalflat/maskflag + layout bytes + spawn list (uint16 per cell) + ball / goal bit strings
    // (v3: two buffers x two planes x one string per group of envs)
    const int grp = (specialised && (G & 1)) ? 4 : 1;
    const size_t marks = (specialised && with_marks) ? (size_t)2 * 2 * (epb / grp) * ((grp * cells + 31) / 32) * 4 : 0;
    return (size_t)pat * 4 + 3 * (size_t)epb * 4 + (size_t)((cells + 15) & ~15) + (size_t)((cells * 2 + 15) & ~15) + marks;
}

int perenv_envs_per_block(int G, int layout_bytes) {
    const int cells = G * G;
    int epb = (layout_bytes / cells) & ~15;
    if (epb < 16) epb = 16;
    if (epb > LMAZE_BLOCK) epb = LMAZE_BLOCK;
    return epb;
}

static size_t perenv_lds_bytes(int G, int epb) {
    return (size_t)((epb * G * G + 15) & ~15) + (3 * (size_t)(epb + 1) + 2 * (size_t)epb) * 4;
}


// LDS bytes that make exactly `k` workgroups fit a CU's 160 KiB (midway between the k and
// k+1 thresholds, clear of the allocation granule).
static size_t lds_for_workgroups_per_cu(int k) {
    const size_t cap = 160 * 1024;
    return ((cap / k + cap / (k + 1)) / 2) & ~(size_t)255;
}

// The instantiations of the shared-layout step kernel, X(grid side, selector, envs per workgroup): per grid side the kernel is
// specialised for -- the reference's shipped sizes (12, 14, 18) and BASELINE.json's (8, 11, 32); any other G in [3, 64] takes the
// generic instantiation, side 0 -- the workgroup sizes that launch_hint bits 10-11 = 1 / 2 / 3 name.  About 32 KiB of observation
// per workgroup (8 sixteen-byte stores per lane) was the starting point: measured at G=11 on MI355X (tools/kbench.hip), 64 envs
// (31 KiB) 90-91 us per 1M-env step, 128/256 envs 96-101 us, 32 envs 120 us; the smaller sizes are step_default_sel's.
// The one list behind kSharedSizes (what step_plan chooses from), step_kernel (what is compiled; the per-env LDS kernel takes
// its grid sides from here too) and specialised_grid.
#define LMAZE_SHARED_SIZES(X)                      \
    X(8, 1, 128) X(8, 2, 64)                       \
    X(11, 1, 64) X(11, 2, 32) X(11, 3, 16)         \
    X(12, 1, 64) X(12, 2, 32) X(12, 3, 16)         \
    X(14, 1, 32) X(14, 2, 16)                      \
    X(18, 1, 32) X(18, 2, 16)                      \
    X(32, 1, 8) X(32, 2, 4)                        \
    X(0, 1, 256) X(0, 2, 64) X(0, 3, 16) /* three sizes cover [3, 64] */
static const struct { int gt, sel, epb; } kSharedSizes[] = {
#define X(GT, SEL, EPB) {GT, SEL, EPB},
    LMAZE_SHARED_SIZES(X)
#undef X
};

static bool specialised_grid(int g) {
#define X(GT, SEL, EPB) || (GT != 0 && g == GT)
    return false LMAZE_SHARED_SIZES(X);
#undef X
}

// Launch policy of the streaming (non-temporal) regime, measured on MI355X with
// tools/kbench.hip (one process, interleaved rounds), workgroups per CU = 8 (no cap) / 4 / 3 / 2:
//   1M x 11x11 (546 MB)   99-101 / 91-97 / 78-79 / 102 us     4M x 11x11   354 / 350 / 320 / 424 us
//   2M x 8x8   (614 MB)   99 / 97 / 92 / 88 us                128K x 32x32   99 / 96 / 92 / 106 us
//   1M x 12x12, 512K x 18x18: flat within 3 %
// i.e. up to 6.9 TB/s instead of 5.5 when only 12 waves per CU stream their 32-KiB chunks (more
// resident waves queue more non-temporal stores than the memory side drains efficiently; with
// plain stores the cap hurts).  The optimum is narrow and shifts with shape and device, so the
// caller can override it: LmazeParams.launch_hint bits 0-3 = workgroups per CU (0 = this
// default), which LmazeVecEnv.autotune() picks by timing real steps.
// ---- the default launch policy of the streaming regime is DATA: lmaze_policy_table.h, generated by tools/gen_policy.py
// from sweeps recorded on MI355X boxes (profiles/rNN/shape_sweep_*.jsonl), looked up by grid side, rules, fused reset and
// the nearest batch size in log2.  sel = the envs-per-workgroup selector of launch_hint bits 10-11 (0: the table's default
// one).  tests/test_gpu_policy_guard.py checks the table's choice against a small sweep on the box it runs on.
static const StepPolicyRow* step_policy_lookup(int g, int variant, bool auto_reset, int64_t n, int sel) {
    const StepPolicyRow* best = nullptr;
    long best_cost = 0;
    const int l2 = (int)lround(log2((double)(n < 1 ? 1 : n)) * 16.0);
    for (int i = 0; i < kStepPolicyRows; ++i) {
        const StepPolicyRow& r = kStepPolicy[i];
        if ((r.auto_reset != 0) != auto_reset) continue;
        if (sel == 0 ? !r.is_default : r.sel != sel) continue;
        if (specialised_grid(g) != specialised_grid(r.g)) continue;
        if (specialised_grid(g) && r.g != g) continue;
        // lexicographic: grid distance (unspecialised G only), then rules, then batch size
        const long cost = (long)abs(r.g - g) * 1000000 + (r.variant != variant ? 100000 : 0) + abs(r.log2n_x16 - l2);
        if (!best || cost < best_cost) { best = &r; best_cost = cost; }
    }
    return best;
}

// the table's default envs-per-workgroup selector for this launch (streaming regime), or `fallback`
static int table_sel(const StepArgs& a, int variant, int fallback) {
    const StepPolicyRow* r = step_policy_lookup(a.grid, variant, a.auto_reset != 0, a.n, 0);
    return r ? r->sel : fallback;
}

// The shared-layout kernel's selector where launch_hint bits 10-11 leave it to the library.  gt: the grid side of the
// instantiation; streaming: the planes go beyond the caches.
static int step_default_sel(const StepArgs& a, int variant, int gt, bool streaming) {
    const bool v3 = variant == LMAZE_VARIANT_V3;
    switch (gt) {
        case 8:
            // large 8x8 batches: 1: 128 envs per workgroup, 2: 64 (16 KiB of planes).  2M envs: 64 envs at
            // 4 / 5 / 6 / 8 per CU 89.0 / 91.7 / 91.8 / 91.7 us, 128 envs at (2, 1) 92.6, at 3-8 per CU 102-105.
            return table_sel(a, variant, a.obs != nullptr ? 2 : 1);
        case 11:
            // envs per workgroup, 1: 64, 2: 32.  Round 2, once the set-up was one global
            // round trip: v0 11x11 1M, 32 envs (15 KiB of planes) per workgroup, uncapped, one chunk 76.1-76.6 us on every
            // placement of the observation buffer tried, against 78.6-80.9 for 64 envs at (3, 2) / (3, 1) (16 envs: 90+);
            // with the fused reset (after its set-up lost the compacted spawn list and the early wait) 32 envs uncapped 78.8-83.5
            // on two boxes, 64 envs at (3, 2) 81 / 95-97, at (3, 1) 81-84.
            return streaming ? table_sel(a, variant, 2) : 1;     // the render-only launches (lmaze_observe) write the same stream
        case 12:
            // 12x12 (1M envs, 643 MB): 16 envs (9 KiB) per workgroup, uncapped 97.1-97.4 us, (5, 2) 96.0, against 104-105 for 64
            // envs at (2, 1) and 111-119 for nearly everything else; with the fused reset 103-104 against 109.  (3: 16 envs.)
            return streaming ? table_sel(a, variant, 3) : 1;
        case 14:
        case 18:
            // envs per workgroup, 1: 32, 2: 16.  1M x 14x14 v0 (861 MB): 16 envs (12 KiB
            // of planes) at 5 workgroups per CU 120.5 us, at 4 / 6 / uncapped 134 / 142 / 142, against 150-161 for every
            // policy of 32 envs but (2, 2) (132.5); 512K x 18x18 v3: 16 envs at (4, 1) or (3, 2) 104.3-104.5 against 109.5
            // for 32 at (2, 1) -- but 118-134 one step to either side, so there it stays a tuner candidate.
            // v3 18x18 since its render went to bit strings: 16 envs at 4-5 per CU 109 us (with the fused reset 5-8 per CU
            // 103-107) against 112-120
            return streaming ? table_sel(a, variant, gt == 14 || v3 ? 2 : 1) : 1;
        case 32:
            // 1: 8 envs per workgroup (32 KiB of planes), 2: 4 envs (16 KiB).  128K / 512K envs, us per
            // step: 4 envs at (5, 1) 84.0 / 337 and at (4, 1) 85.0 / 323 against 96 / 363 for 8 envs at (2, 1); with the fused
            // reset 4 envs at (5, 1) 88.6 / 342, at (6, 1) 81.8 / 313, against 102 / 403.
            return streaming ? table_sel(a, variant, 2) : 1;
        default: {
            // unspecialised G: 1: 256, 2: 64, 3: 16 envs per workgroup.
            // Round 2 (1M envs at G = 9, 10, 13; 512K at 16, 20; 256K at 27; us per step, old -> new default): 64.9 -> 56.4,
            // 88.0 -> 76.2, 120.7 (unchanged), 118.9 -> 90.0 (16 envs at (5, 2): 81.7), 169.7 -> 148.1, 155.3 -> 152.
            const int sel = a.grid >= 15 ? 3 : (a.grid >= 5 ? 2 : 1);
            return streaming && a.grid >= 5 ? table_sel(a, variant, sel) : sel;
        }
    }
}

// What a step / observe launch queues (step_plan): everything the description and the launch need
enum StepFamily { ST_SHARED, ST_WAVE8, ST_PERENV, ST_PERENV_WAVE, ST_U8 };
struct StepPlan {
    StepFamily family;
    int gt;                   // the instantiation's grid side (0: the generic one; wave8 and u8 have none)
    int epb;                  // ... and its envs per workgroup (wave8: per wave; the per-env kernels have none)
    bool nt;                  // the instantiation with non-temporal stores
    int envs;                 // reported: envs per workgroup
    int per_cu;               // reported: the workgroups per CU the LDS request asks for, 0 without a cap
    int chunks;
    int64_t grid;
    int block;
    size_t lds;
    int32_t envs_per_block;   // what the kernel receives as StepArgs::envs_per_block (the per-env kernels') ...
    int32_t launch_hint;      // ... and as launch_hint (the u8 kernel's bit 8: streaming stores)
};

// narrow (uint8) observation: envs per workgroup 256 and two chunks of them unless the hint says otherwise
static const int kU8DefaultSel = 1, kU8DefaultChunks = 2;

static StepPlan step_plan(const StepArgs& a, int variant, int layout_mode, bool u8) {
    const int cells = a.grid * a.grid;
    const int hint_sel = (a.launch_hint >> 10) & 3, hint_lo = a.launch_hint & 15, hint_hi = (a.launch_hint >> 4) & 15;
    const bool streaming = a.obs != nullptr && beyond_caches(a.n, cells);
    StepPlan p{ST_SHARED, 0, 0, false, 0, 0, 1, 0, LMAZE_BLOCK, 0, a.envs_per_block, a.launch_hint};
    if (u8) {
        // shared layout.  launch_hint bits 10-11: envs per workgroup, 1: 256, 2: 128, 3: 64 (0 = default)
        p.family = ST_U8;
        p.envs = p.epb = 512 >> (hint_sel ? hint_sel : kU8DefaultSel);
        const int pw = (2 * cells + 16 + 3) >> 2;
        p.lds = ((size_t)4 * pw * 4 + 3 * (size_t)(p.epb + 1) * 4 + (size_t)((cells + 1) & ~1) * 2 + (size_t)cells + 15) & ~(size_t)15;
        // launch_hint bits 4-7: chunks of epb envs per workgroup (0 = default)
        p.chunks = hint_hi ? hint_hi : kU8DefaultChunks;
        p.grid = ((a.n + p.epb - 1) / p.epb + p.chunks - 1) / p.chunks;
        // more than 64 MiB of planes: streamed (1M x 11x11, 127 MB: 31.2 us per step against 33.3 with plain stores)
        p.launch_hint = (a.launch_hint & ~0x100) | ((size_t)a.n * cells > ((size_t)64 << 20) ? 0x100 : 0);
    } else if (layout_mode != LMAZE_LAYOUT_SHARED && cells % 256 == 0) {
        // G*G a multiple of 256 (16, 32, 48, 64): the register-tiled one-wave-per-env kernel.
        // One env per wave measured best at 1M x 32x32 (bench.py --workload c5): 0.873 ms per step
        // (0.775 of HBM peak, non-temporal stores) against 0.985 ms with four envs per wave and 0.96 ms
        // for the LDS-tiled kernel -- short-lived waves, as with the one-store-per-thread fill.
        p.family = ST_PERENV_WAVE;
        p.gt = a.grid;
        p.nt = streaming;
        p.envs_per_block = 1;
        p.envs = p.envs_per_block * (LMAZE_BLOCK / 64);
        p.grid = (a.n + p.envs - 1) / p.envs;
    } else if (layout_mode != LMAZE_LAYOUT_SHARED) {
        p.family = ST_PERENV;
        p.gt = specialised_grid(a.grid) ? a.grid : 0;
        // about 8 KiB of layouts = 32 KiB of planes per workgroup (round 1: 16 KiB; 1M x 11x11 / 12x12, 512K x 18x18 with
        // non-temporal stores: 107 / 125 / 134 us with 16 KiB, 102-103 / 120-122 / 133-140 with 8)
        p.envs = p.envs_per_block = perenv_envs_per_block(a.grid, 8192);
        p.grid = (a.n + p.envs - 1) / p.envs;
        p.lds = perenv_lds_bytes(a.grid, p.envs);
    } else if (a.grid == 8 && !streaming && a.mask == nullptr && (a.launch_hint & 0x100) == 0) {
        // small 8x8 batches (the planes stay on-die): the wave-autonomous kernel, no LDS, no barrier
        // envs per wave: launch_hint bits 4-7 = 1: 64, 2: 32, 3: 16 (0 = default)
        // Defaults, measured at 65 536 envs under hipGraph (us per step, two boxes): 64 envs per wave x 4 waves per
        // workgroup -- one 256-thread workgroup per CU -- 5.35-5.53; 64 x 1 5.6-5.9; 32 x 1 / 2 / 4 5.72 / 5.72-5.87 /
        // 5.89; 64 x 2 5.9-6.1.  Smaller batches keep single-wave workgroups so that they spread over the CUs.
        p.family = ST_WAVE8;
        p.epb = 128 >> (hint_hi >= 1 && hint_hi <= 3 ? hint_hi : a.n >= 65536 ? 1 : 2);
        // bits 0-3: waves per workgroup, 1 / 2 / 4 (0 = default)
        const int wpb = hint_lo == 1 || hint_lo == 2 || hint_lo == 4 ? hint_lo : a.n >= 65536 ? 4 : 1;
        p.envs = p.epb * wpb;
        p.block = 64 * wpb;
        p.grid = ((a.n + p.epb - 1) / p.epb + wpb - 1) / wpb;
    } else {
        // launch_hint bits 10-11 name the envs per workgroup (0 = default); a selector the grid side has no size for takes
        // selector 1's
        p.gt = specialised_grid(a.grid) ? a.grid : 0;
        auto size_of = [&](int sel) {
            for (const auto& size : kSharedSizes)
                if (size.gt == p.gt && size.sel == sel) return size.epb;
            return 0;
        };
        int sel = hint_sel ? hint_sel : step_default_sel(a, variant, p.gt, streaming);
        if (!size_of(sel)) sel = 1;
        p.envs = p.epb = size_of(sel);
        p.nt = streaming;
        p.lds = shared_lds_bytes(a.grid, p.gt != 0, p.epb, variant == LMAZE_VARIANT_V3);
        // default (workgroups per CU, chunks per workgroup) of the streaming regime: the generated table's row for the chosen
        // size (round 2 kept them in a hand-edited if-chain here, retuned four times in its last hour; LAB_NOTES.md has that
        // history).  Inside the caches neither default is read.
        int def_cu = 3, def_m = 2;
        const StepPolicyRow* r = p.nt ? step_policy_lookup(a.grid, variant, a.auto_reset != 0, a.n, sel) : nullptr;
        if (r) {
            def_cu = r->per_cu;
            def_m = r->chunks;
        }
        const int per_cu = hint_lo == 0 && p.nt ? def_cu : hint_lo;
        if (per_cu >= 1 && per_cu < 8) {
            p.per_cu = per_cu;
            const size_t want = lds_for_workgroups_per_cu(per_cu);
            if (want > p.lds) p.lds = want;
        }
        // chunks per workgroup (hint bits 4-7, 0 = default): the inputs of chunk k+1 are loaded while chunk k is
        // stored, and the per-workgroup LDS set-up is shared.
        p.chunks = hint_hi ? hint_hi : p.nt ? def_m : 1;
        p.grid = ((a.n + p.epb - 1) / p.epb + p.chunks - 1) / p.chunks;
    }
    return p;
}

// The kernel of a planned step: every instantiation the code object holds is named here and nowhere else
using StepKernel = void (*)(const StepArgs);
template <int V, bool S>
static StepKernel step_kernel(const StepPlan& p) {
    switch (p.family) {
        case ST_SHARED:
#define X(GT, SEL, EPB) \
    if (p.gt == GT && p.epb == EPB) return p.nt ? step_shared_kernel<GT, V, S, EPB, true> : step_shared_kernel<GT, V, S, EPB, false>;
            LMAZE_SHARED_SIZES(X)
#undef X
            break;
        case ST_PERENV:   // side 32 always takes the wave kernel; its instantiation stays in the code object
#define X(GT, SEL, EPB) \
    if (SEL == 1 && p.gt == GT) return step_perenv_kernel<GT, V, S>;
            LMAZE_SHARED_SIZES(X)
#undef X
            break;
        case ST_PERENV_WAVE:
#define X(G) \
    if (p.gt == G) return p.nt ? step_perenv_wave_kernel<G, V, S, true> : step_perenv_wave_kernel<G, V, S, false>;
            X(16) X(32) X(48) X(64)
#undef X
            break;
        case ST_WAVE8:
            return p.epb == 64 ? step_shared_wave8_kernel<V, S, 64> : p.epb == 32 ? step_shared_wave8_kernel<V, S, 32> : step_shared_wave8_kernel<V, S, 16>;
        case ST_U8:
            return p.epb == 256 ? step_shared_u8_kernel<V, S, 256> : p.epb == 128 ? step_shared_u8_kernel<V, S, 128> : step_shared_u8_kernel<V, S, 64>;
    }
    return nullptr;
}

static const void* step_kernel(const StepPlan& p, bool v3, bool do_step) {
    constexpr int V0 = LMAZE_VARIANT_V0, V3 = LMAZE_VARIANT_V3;
    return (const void*)(v3 ? (do_step ? step_kernel<V3, true>(p) : step_kernel<V3, false>(p))
                            : (do_step ? step_kernel<V0, true>(p) : step_kernel<V0, false>(p)));
}

// One step (do_step) or one render (observe) of a.n envs as step_plan decides; u8: the narrow planes in a.obs8 (shared layouts,
// G >= 4).  a.info != null: the plan is described instead of queued.
hipError_t launch_step(int variant, bool do_step, const StepArgs& a, int layout_mode, bool u8, hipStream_t s) {
    if (a.n == 0) return hipSuccess;
    const bool v3 = variant == LMAZE_VARIANT_V3;
    const StepPlan p = step_plan(a, v3 ? LMAZE_VARIANT_V3 : LMAZE_VARIANT_V0, layout_mode, u8);
    if (!grid_ok(p.grid)) return hipErrorInvalidConfiguration;
    if (a.info) {
        char name[96];
        const char *v = v3 ? "v3" : "v0", *form = do_step ? "step" : "observe", *stores = p.nt ? "nt" : "plain";
        switch (p.family) {
            case ST_SHARED: snprintf(name, sizeof(name), "step_shared_kernel<%d, %s, %s, %d, %s>", p.gt, v, form, p.epb, stores); break;
            case ST_PERENV: snprintf(name, sizeof(name), "step_perenv_kernel<%d, %s, %s>", p.gt, v, form); break;
            case ST_PERENV_WAVE: snprintf(name, sizeof(name), "step_perenv_wave_kernel<%d, %s, %s, %s>", p.gt, v, form, stores); break;
            case ST_WAVE8: snprintf(name, sizeof(name), "step_shared_wave8_kernel<%s, %s, %d>", v, form, p.epb); break;
            case ST_U8: snprintf(name, sizeof(name), "step_shared_u8_kernel<%s, %s, %d>", v, form, p.epb); break;
        }
        describe_launch(a.info, name, p.envs, p.per_cu, p.chunks, p.nt, p.grid, p.block, p.lds);
        return hipSuccess;
    }
    StepArgs b = a;
    b.envs_per_block = p.envs_per_block;
    b.launch_hint = p.launch_hint;
    void* args[] = {&b};
    (void)hipLaunchKernel(step_kernel(p, v3, do_step), dim3((unsigned)p.grid), dim3(p.block), args, p.lds, s);   // read back as after hipLaunchKernelGGL
    return hipGetLastError();
}

// Store policy of the recording form's slots: plain.  Measured (tools/bench_rollout_obs.py --sweep, two runs, T = 16,
// every step recorded; launch_hint bit 15 = non-temporal, for measurement -- results never change), us per step plain / nt:
//   65 536 x 11x11 shared (507 MB of slots, beyond the 256-MiB Infinity Cache)   6.2-6.5 / 7.2-7.5
//   1M x 11x11 shared (8.1 GB)  109.5-110.4 / 110.5-110.7     262 144 x 32x32 per-env (17 GB)  219.5-223.9 / 221.1-222.3
//   16 384 x 11x11 per-env (127 MB, inside it)  4.0 / 3.8 at 16 envs per workgroup (plain runs spread 3.7-4.8)
// i.e. streaming wins nothing beyond a few per cent inside the cache and loses 12-18 % where the slots are about twice
// the cache.  The wave-autonomous 8x8 form has no choice: with it, it spills at its twin's 6 waves per SIMD.
static bool slot_stores_nt(const StepArgs& a, const RolloutRec* rec) {
    return rec && rec->obs_t && ((a.launch_hint >> 15) & 1);
}

// What a grid rollout queues (rollout_plan): one launch of a rollout kernel -- the family, its envs per workgroup, block,
// blocks, LDS and slot store policy -- or T launches of the step kernel
enum RolloutFamily { RO_WAVE8, RO_SHARED, RO_PERENV, RO_U8, RO_STEPS };
static const char* const kRolloutKernel[] = {"rollout_shared_wave8_kernel", "rollout_shared_kernel", "rollout_perenv_kernel",
                                             "rollout_shared_u8_kernel"};
struct RolloutPlan {
    RolloutFamily family;
    int epb;                  // envs per workgroup (wave8: envs per wave x waves per workgroup)
    int block;
    int64_t blocks;
    size_t lds;
    bool nt;                  // the recording form's slot stores: non-temporal
};

// T >= 1 steps of a.n >= 1 envs (rec != null: the recording form; u8: the narrow planes, shared layouts).  int32 planes: ONE
// launch (shared layouts: rollout_shared_wave8_kernel for on-die 8x8, rollout_shared_kernel otherwise; per-env layouts:
// rollout_perenv_kernel); T launches of the step kernel only for T = 1 or when launch_hint bit 8 forces streaming stores.
// u8: ONE launch of rollout_shared_u8_kernel for any T and any batch size.
// pol: the table kind of lmaze_rollout_lds.h, which says what each body keeps in LDS and where (LMAZE_TAB_ENV_BYTES: as many
// bytes again as the layouts -- the 32-KiB rule stays on the layouts, the 160-KiB clamp is on the total).  Not LMAZE_TAB_NONE: the
// closed-loop forms (rec != null) -- always one launch of a workgroup kernel (no T-launch fallback, no wave8 form: on-die
// 8x8 goes through rollout_shared_kernel), the recording form's envs per workgroup, and the table in every LDS size, the
// fits and clamps below included.
static RolloutPlan rollout_plan(const StepArgs& a, int layout_mode, int32_t T, const RolloutRec* rec, bool u8, int pol = LMAZE_TAB_NONE) {
    const int cells = a.grid * a.grid;
    const int hint_epb = (a.launch_hint >> 12) & 7;       // bits 12-14 = k > 0 ask for 4 << (k - 1) envs per workgroup
    // the recording form streams its slots wherever the batch sits; on-die means the batch's planes fit the caches
    const bool planes = a.obs != nullptr || (rec && rec->obs_t);
    RolloutPlan p{RO_STEPS, 0, LMAZE_BLOCK, 0, 0, false};
    if (u8) {
        // launch_hint bits 12-14 rounded up to 16 (a workgroup's byte range of obs8 must start on a 16-byte boundary) and down
        // to what fits 64 KiB of LDS; performance only.  Bit 8 keeps its one meaning of the u8 step (streaming stores there)
        // and is not read here.  Envs per workgroup, from tools/bench_rollout_u8.py --sweep (v0, fused reset, T = 16, us per
        // step for 16 / 32 / 64 / 128 / 256 envs; plain rollout, then every step recorded;
        // profiles/rollout_u8/bench_rollout_u8_sweep.json):
        //   65 536 x 8x8     3.41 / 2.54 / 1.90 / 2.08 / 2.31      4.70 / 3.33 / 2.46 / 2.49 / 2.71
        //   65 536 x 11x11   3.94 / 2.93 / 2.46 / 2.79 / 3.70      5.18 / 3.63 / 3.00 / 3.24 / 4.04
        //   16 384 x 12x12   1.66 / 1.77 / 1.95 / 2.28 / 2.98      2.16 / 2.20 / 2.27 / 2.57 / 3.34
        //   262 144 x 11x11  11.5 / 7.08 / 5.70 / 7.07 / 7.07      17.3 / 12.1 / 9.50 / 8.88 / 7.78
        //   1M x 11x11       42.8 / 25.7 / 19.5 / 24.6 / 25.5      73.8 / 51.6 / 39.3 / 29.4 / 29.0
        // i.e. 64 envs from 65 536 envs on and 16 below; the slots of a recording beyond the Infinity Cache (262 144 x 11x11 x
        // 16 slots = 507 MB) want the widest workgroups.  The int32 rule of fitting the resident workgroups' planes into L2
        // does not carry over: 1M x 11x11 with 16 envs is 2.2x slower than with 64.
        int epb = a.n >= 65536 ? 64 : 16;
        if (rec && rec->obs_t && a.n >= 262144) epb = 256;
        if (hint_epb) epb = 4 << (hint_epb - 1);
        if (epb < 16) epb = 16;
        if (epb > LMAZE_BLOCK) epb = LMAZE_BLOCK;
        while (epb > 16 && lmaze_rollout_lds_u8(cells, epb, pol).total > (64 << 10)) epb >>= 1;
        p.family = RO_U8;
        p.epb = epb;
        p.lds = (size_t)lmaze_rollout_lds_u8(cells, epb, pol).total;
    } else if (!pol && layout_mode == LMAZE_LAYOUT_SHARED && a.grid == 8 && (!planes || !beyond_caches(a.n, 64)) &&
               (a.launch_hint & 0x100) == 0) {
        // on-die 8x8: 64 envs per wave, one wave per workgroup below 65 536 envs and 4 from there on
        p.family = RO_WAVE8;
        p.block = 64 * (a.n >= 65536 ? 4 : 1);
        p.epb = p.block;
    } else if (pol || (T > 1 && (a.launch_hint & 0x100) == 0)) {
        const bool perenv = layout_mode == LMAZE_LAYOUT_PER_ENV;
        p.family = perenv ? RO_PERENV : RO_SHARED;
        // shared layouts: a workgroup per 16 / 32 / 64 envs so that small batches still fill the chip.  Streaming sizes too:
        // the planes of every step still go out to HBM, but the state stays in registers and there is no per-step set-up --
        // 1M x 11x11 75.4 us per step (fused reset 75.6) against 86.4 (92.5) as T launches from inside this call, 4M envs
        // 297.8 against 329.7 (profiles/r03/rollout_streaming.txt).  Per-env layouts, any size: the layouts are read ONCE
        // per rollout instead of once per step (1M x 32x32: 838 -> 722 us per step, 1M x 11x11 103 -> 100.5, with the fused
        // reset 114 -> 105.7, 512K x 18x18 142 -> 114; only 8 192 x 32x32, where the register-tiled step kernel is neither
        // launch- nor layout-bound, is 3 % slower: 10.2 -> 10.5; profiles/r03/rollout_streaming_perenv.txt,
        // rollout_sizes_perenv.txt)
        int epb = a.n >= 65536 ? 64 : (a.n >= 16384 ? 32 : 16);
        if (perenv)
            while (epb > 4 && (size_t)epb * cells > (size_t)32 << 10) epb >>= 1;        // at most 32 KiB of layouts per workgroup
        // Batches whose planes do not fit the caches: few enough envs per workgroup that what the resident workgroups of an XCD
        // rewrite step after step (8 per CU x 32 CUs x envs x 4 G^2 bytes) stays inside its 4-MiB L2 -- then most of the
        // intermediate planes never travel to DRAM.  1M x 11x11: 64 envs 77.7 us per step, 32: 78.6, 16: 51.0, 8: 64.2, 4: 109;
        // 512K x 18x18: 64: 89.2, 16: 98.4, 8: 74.2, 4: 76.2; 256K x 32x32 (no size fits): 146 / 140 / 133.7 / 141.6
        // (profiles/r03/rollout_envs_per_workgroup.txt).
        // (Only beyond the Infinity Cache: 262 144 x 11x11, 127 MB of planes, runs 9.9 us per step at 64 envs and 12.9 at 16.)
        // The recording form keeps the size by batch (launch_hint bits 12-14 swept, T = 16, us per step for every step
        // recorded / final planes only): 1M x 11x11 64 envs 109.1 / 16.2, 32: 109.4 / 21.0, 16 (what the fit picks)
        // 125.7 / 31.5, 8: 147.6 / 52.8; 65 536 x 11x11 64 or 32 6.5-7.8, 8 / 16 7.6-9.7 (profiles/rollout_obs/)
        if (!rec && beyond_caches(a.n, cells))
            while (epb > 8 && (size_t)epb * cells * 4 > 12288) epb >>= 1;
        // the per-env recording form (launch_hint bits 12-14 swept, T = 16, every step recorded): 16 384 x 11x11 16 envs 3.7 us
        // per step, 32 (the plain form's) 4.7, 8 4.4, 64 7.1; 262 144 x 32x32 the plain form's 32 envs 221 us, 16 255,
        // 8 237, 64 346 -- so only the batches that take 32 by size (16 384 to 65 535 envs) halve
        if (perenv && rec && epb == 32 && a.n < 65536) epb = 16;
        if (hint_epb) epb = 4 << (hint_epb - 1);
        if (perenv && epb > 64) epb = 64;                                               // every env's lane sits in wave 0
        // per-env layouts past G = 50 at 64 envs outgrow one workgroup's LDS (the hint is applied after the 32-KiB rule above):
        // halve to what fits, the device's 160 KiB as lds_for_workgroups_per_cu takes it, so that lmaze_describe_rollout
        // answers the same without a device.  Stays a multiple of 4 (body 3 copies the layouts as dwords).
        if (perenv)
            while (epb > 4 && lmaze_rollout_lds_perenv(cells, epb, pol).total > 160 * 1024) epb >>= 1;
        p.epb = epb;
        p.lds = (size_t)(perenv ? lmaze_rollout_lds_perenv(cells, epb, pol) : lmaze_rollout_lds_shared(cells, epb, pol)).total;
        p.nt = slot_stores_nt(a, rec);
    }
    if (p.family != RO_STEPS) p.blocks = (a.n + p.epb - 1) / p.epb;
    return p;
}

// The kernel of a planned rollout, the only place that names a rollout instantiation: by family and variant, and by form an
// overload on its argument struct -- plain RolloutArgs, recording RolloutObsArgs, epsilon-greedy RolloutPolicyArgs, sampling
// RolloutSampleArgs, with a table per env RolloutEnvBytesArgs / RolloutEnvRowsArgs (int32 planes only: never RO_U8); u8:
// RolloutArgs and the *8Args; the Q-learner RolloutEnvQArgs (int32 planes only).  The wave-autonomous family is never planned
// for a closed-loop form.
enum RolloutForm { RF_PLAIN, RF_REC, RF_POLICY, RF_SAMPLE, RF_ENV_POLICY, RF_ENV_SAMPLE, RF_ENV_QLEARN };
template <class Args>
using RolloutFn = void (*)(const StepArgs, const Args);
template <class F>
static const void* kernel_of(int variant, F v3, F v0) { return (const void*)(variant == LMAZE_VARIANT_V3 ? v3 : v0); }

static const void* rollout_kernel(RolloutFamily f, int variant, RolloutForm form) {
    using P = RolloutFn<RolloutArgs>; using R = RolloutFn<RolloutObsArgs>; using R8 = RolloutFn<RolloutObs8Args>;
    using E = RolloutFn<RolloutPolicyArgs>; using E8 = RolloutFn<RolloutPolicy8Args>;
    using S = RolloutFn<RolloutSampleArgs>; using S8 = RolloutFn<RolloutSample8Args>;
    using EB = RolloutFn<RolloutEnvBytesArgs>; using ER = RolloutFn<RolloutEnvRowsArgs>; using EQ = RolloutFn<RolloutEnvQArgs>;
    constexpr int V0 = LMAZE_VARIANT_V0, V3 = LMAZE_VARIANT_V3;
    switch (f) {
        case RO_WAVE8: return form == RF_PLAIN ? kernel_of<P>(variant, rollout_shared_wave8_kernel<V3, 64>, rollout_shared_wave8_kernel<V0, 64>)
                                               : kernel_of<R>(variant, rollout_shared_wave8_kernel<V3, 64>, rollout_shared_wave8_kernel<V0, 64>);
        case RO_SHARED: return form == RF_PLAIN    ? kernel_of<P>(variant, rollout_shared_kernel<V3>, rollout_shared_kernel<V0>)
                               : form == RF_REC    ? kernel_of<R>(variant, rollout_shared_kernel<V3>, rollout_shared_kernel<V0>)
                               : form == RF_POLICY ? kernel_of<E>(variant, rollout_shared_kernel<V3>, rollout_shared_kernel<V0>)
                               : form == RF_SAMPLE ? kernel_of<S>(variant, rollout_shared_kernel<V3>, rollout_shared_kernel<V0>)
                               : form == RF_ENV_POLICY ? kernel_of<EB>(variant, rollout_shared_kernel<V3>, rollout_shared_kernel<V0>)
                               : form == RF_ENV_SAMPLE ? kernel_of<ER>(variant, rollout_shared_kernel<V3>, rollout_shared_kernel<V0>)
                                                       : kernel_of<EQ>(variant, rollout_shared_kernel<V3>, rollout_shared_kernel<V0>);
        case RO_PERENV: return form == RF_PLAIN    ? kernel_of<P>(variant, rollout_perenv_kernel<V3>, rollout_perenv_kernel<V0>)
                               : form == RF_REC    ? kernel_of<R>(variant, rollout_perenv_kernel<V3>, rollout_perenv_kernel<V0>)
                               : form == RF_POLICY ? kernel_of<E>(variant, rollout_perenv_kernel<V3>, rollout_perenv_kernel<V0>)
                               : form == RF_SAMPLE ? kernel_of<S>(variant, rollout_perenv_kernel<V3>, rollout_perenv_kernel<V0>)
                               : form == RF_ENV_POLICY ? kernel_of<EB>(variant, rollout_perenv_kernel<V3>, rollout_perenv_kernel<V0>)
                               : form == RF_ENV_SAMPLE ? kernel_of<ER>(variant, rollout_perenv_kernel<V3>, rollout_perenv_kernel<V0>)
                                                       : kernel_of<EQ>(variant, rollout_perenv_kernel<V3>, rollout_perenv_kernel<V0>);
        default: return form == RF_PLAIN    ? kernel_of<P>(variant, rollout_shared_u8_kernel<V3>, rollout_shared_u8_kernel<V0>)
                        : form == RF_REC    ? kernel_of<R8>(variant, rollout_shared_u8_kernel<V3>, rollout_shared_u8_kernel<V0>)
                        : form == RF_POLICY ? kernel_of<E8>(variant, rollout_shared_u8_kernel<V3, true>, rollout_shared_u8_kernel<V0, true>)
                                            : kernel_of<S8>(variant, rollout_shared_u8_kernel<V3, true>, rollout_shared_u8_kernel<V0, true>);
    }
}

// The one launch site of the one-launch rollouts: plan p of form `form` with the kernel's second argument ro (the form's
// struct), queued -- or, a0.info != null, described under `name`
static hipError_t launch_planned(const RolloutPlan& p, int variant, RolloutForm form, const StepArgs& a0, void* ro, const char* name,
                                 hipStream_t s) {
    if (!grid_ok(p.blocks)) return hipErrorInvalidConfiguration;
    if (a0.info) {
        describe_launch(a0.info, name, p.epb, 0, 1, p.nt, p.blocks, p.block, p.lds);
        return hipSuccess;
    }
    StepArgs a = a0;
    a.envs_per_block = p.epb;
    void* args[] = {&a, ro};
    (void)hipLaunchKernel(rollout_kernel(p.family, variant, form), dim3((unsigned)p.blocks), dim3(p.block), args, p.lds, s);   // read back as after hipLaunchKernelGGL
    return hipGetLastError();
}

// T steps as rollout_plan decides.  T launches: step t with the action row t, epoch + t and, when given, the per-step
// reward / done rows copied out; recording, each step gets its slot, the caller's obs (last step) or nothing.
hipError_t launch_rollout(int variant, const StepArgs& a0, int layout_mode, const ActionRows& src, int32_t T, float* reward_t,
                          uint8_t* done_t, hipStream_t s, const RolloutRec& request, bool u8) {
    if (T <= 0 || a0.n == 0) return hipSuccess;
    const RolloutRec* rec = src.recording ? &request : nullptr;
    const RolloutPlan p = rollout_plan(a0, layout_mode, T, rec, u8);
    if (p.family == RO_STEPS) {
        int32_t* obs_t = rec ? static_cast<int32_t*>(rec->obs_t) : nullptr;
        const int64_t plane = (int64_t)a0.n * a0.grid * a0.grid;                    // dwords of one step's planes
        for (int32_t t = 0; t < T; ++t) {
            StepArgs a = a0;
            a.action = src.actions + (size_t)t * a0.n;
            a.epoch = a0.epoch + (uint64_t)t;
            int32_t* slot = nullptr;                                                 // recording: the slot step t fills
            if (obs_t && rec->every > 0 && (t + 1) % rec->every == 0)
                slot = obs_t + (size_t)((t + 1) / rec->every - 1) * plane;
            if (rec) a.obs = t == T - 1 && a0.obs ? a0.obs : slot;                     // the caller's obs after the last step
            hipError_t rc = launch_step(variant, true, a, layout_mode, u8, s);
            if (rc != hipSuccess || a0.info) return rc;
            if (slot && a.obs != slot && (rc = hipMemcpyAsync(slot, a.obs, (size_t)plane * 4, hipMemcpyDeviceToDevice, s)) != hipSuccess)
                return rc;
            if (reward_t && (rc = hipMemcpyAsync(reward_t + (size_t)t * a0.n, a0.reward, (size_t)a0.n * 4, hipMemcpyDeviceToDevice, s)) != hipSuccess) return rc;
            if (done_t && (rc = hipMemcpyAsync(done_t + (size_t)t * a0.n, a0.done, (size_t)a0.n, hipMemcpyDeviceToDevice, s)) != hipSuccess) return rc;
        }
        return hipSuccess;
    }
    char name[96] = "", every[24] = "";
    if (a0.info) {
        if (rec) snprintf(every, sizeof(every), " every=%d", rec->every);
        snprintf(name, sizeof(name), "%s<v%d%s%s%s> T=%d%s", kRolloutKernel[p.family], variant, p.family == RO_WAVE8 ? ", 64" : "",
                 rec ? ", obs_t" : "", p.nt ? ", nt" : "", T, every);
    }
    RolloutArgs plain{src.actions, reward_t, done_t, T};
    RolloutObsArgs ro{plain, rec ? static_cast<int32_t*>(rec->obs_t) : nullptr, rec ? rec->every : 0, p.nt ? 1 : 0};
    RolloutObs8Args ro8{plain, rec ? static_cast<uint8_t*>(rec->obs_t) : nullptr, rec ? rec->every : 0};
    return launch_planned(p, variant, rec ? RF_REC : RF_PLAIN, a0, !rec ? (void*)&plain : u8 ? (void*)&ro8 : (void*)&ro, name, s);
}

// The closed-loop rollouts: ONE launch of the planned family's closed-loop form, whatever T and launch_hint bit 8 say.
// Args / Args8: the kernel argument structs that carry `tab` (int32 / narrow planes); kind: the LMAZE_TAB_* of the form,
// which the describe name states as "<policy|sample|qlearn>=<ball|goal|env>[, table=<lds|global>]".  Args8 void: the form has no narrow planes.
static const char* key_name(const PolicyTable& t) { return t.key_mode ? "goal" : "ball"; }
static const char* key_name(const SampleTable& t) { return t.key_mode ? "goal" : "ball"; }
static const char* key_name(const EnvPolicyTable&) { return "env"; }
static const char* key_name(const EnvSampleTable&) { return "env"; }
static const char* key_name(const EnvQTable&) { return "env"; }
template <class Args, class Args8, class Table>
static hipError_t launch_closed(int variant, const StepArgs& a0, int layout_mode, const Table& tab, int kind, RolloutForm form, int32_t T,
                                float* reward_t, uint8_t* done_t, hipStream_t s, const RolloutRec& rec, bool u8) {
    if (T <= 0 || a0.n == 0) return hipSuccess;
    const RolloutPlan p = rollout_plan(a0, layout_mode, T, &rec, u8, kind);
    char name[96] = "";
    if (a0.info)
        snprintf(name, sizeof(name), "%s<v%d, %s=%s%s%s%s> T=%d every=%d", kRolloutKernel[p.family], variant,
                 form == RF_POLICY || form == RF_ENV_POLICY ? "policy" : form == RF_ENV_QLEARN ? "qlearn" : "sample", key_name(tab),
                 kind == LMAZE_TAB_ROWS || kind == LMAZE_TAB_ENV_BYTES ? ", table=lds" : kind == LMAZE_TAB_GLOBAL ? ", table=global" : "",
                 rec.obs_t ? ", obs_t" : "", p.nt ? ", nt" : "", T, rec.every);
    RolloutArgs plain{nullptr, reward_t, done_t, T};
    Args ro{{plain, static_cast<int32_t*>(rec.obs_t), rec.every, p.nt ? 1 : 0}, tab};
    if constexpr (!std::is_void<Args8>::value) {
        Args8 ro8{{plain, static_cast<uint8_t*>(rec.obs_t), rec.every}, tab};
        if (u8) return launch_planned(p, variant, form, a0, &ro8, name, s);
    }
    return launch_planned(p, variant, form, a0, &ro, name, s);
}

// lmaze_env_rollout_policy: per-env layouts stage the workgroup's tables in LDS (counted where rollout_plan fits and clamps the
// envs per workgroup); shared layouts read them from global memory
hipError_t launch_rollout(int variant, const StepArgs& a, int layout_mode, const EnvPolicyTable& tab, int32_t T, float* reward_t,
                          uint8_t* done_t, hipStream_t s, const RolloutRec& rec, bool) {
    const int kind = layout_mode == LMAZE_LAYOUT_PER_ENV ? LMAZE_TAB_ENV_BYTES : LMAZE_TAB_GLOBAL;
    return launch_closed<RolloutEnvBytesArgs, void>(variant, a, layout_mode, tab, kind, RF_ENV_POLICY, T, reward_t, done_t, s, rec, false);
}

// lmaze_env_rollout_sample: the rows stay in global memory
hipError_t launch_rollout(int variant, const StepArgs& a, int layout_mode, const EnvSampleTable& tab, int32_t T, float* reward_t,
                          uint8_t* done_t, hipStream_t s, const RolloutRec& rec, bool) {
    return launch_closed<RolloutEnvRowsArgs, void>(variant, a, layout_mode, tab, LMAZE_TAB_GLOBAL, RF_ENV_SAMPLE, T, reward_t, done_t, s, rec, false);
}

// lmaze_env_rollout_qlearn: the Q rows are read and written in global memory, nothing of them in LDS
hipError_t launch_rollout(int variant, const StepArgs& a, int layout_mode, const EnvQTable& tab, int32_t T, float* reward_t,
                          uint8_t* done_t, hipStream_t s, const RolloutRec& rec, bool) {
    return launch_closed<RolloutEnvQArgs, void>(variant, a, layout_mode, tab, LMAZE_TAB_GLOBAL, RF_ENV_QLEARN, T, reward_t, done_t, s, rec, false);
}

// lmaze_rollout_policy / _u8: the epsilon-greedy table, always staged
hipError_t launch_rollout(int variant, const StepArgs& a, int layout_mode, const PolicyTable& tab, int32_t T, float* reward_t,
                          uint8_t* done_t, hipStream_t s, const RolloutRec& rec, bool u8) {
    return launch_closed<RolloutPolicyArgs, RolloutPolicy8Args>(variant, a, layout_mode, tab, LMAZE_TAB_BYTES, RF_POLICY, T, reward_t, done_t, s, rec, u8);
}

// lmaze_rollout_sample / _u8: the threshold table is staged in LDS by rule -- ball-keyed and G <= 32, i.e. at most 16 KiB --
// and read from global memory otherwise
hipError_t launch_rollout(int variant, const StepArgs& a, int layout_mode, const SampleTable& tab0, int32_t T, float* reward_t,
                          uint8_t* done_t, hipStream_t s, const RolloutRec& rec, bool u8) {
    SampleTable tab = tab0;
    tab.staged = tab.key_mode == 0 && a.grid <= 32 ? 1 : 0;
    const int kind = tab.staged ? LMAZE_TAB_ROWS : LMAZE_TAB_GLOBAL;
    return launch_closed<RolloutSampleArgs, RolloutSample8Args>(variant, a, layout_mode, tab, kind, RF_SAMPLE, T, reward_t, done_t, s, rec, u8);
}

}  // namespace lmaze
