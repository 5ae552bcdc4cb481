/*
 * lmaze.h -- C ABI of the MI355X-native batched L-maze step path (liblmaze_hip.so).
 *
 * The reference (gkm2708/gym-lmaze) has no FFI: its hot path is the body of each env
 * class's step()/reset() in pure Python.  This header is the boundary a maintainer of
 * the reference would bind instead of those bodies (ctypes stub in INTEGRATION.md).
 * Every entry point names the reference lines it replaces; "v0" below means
 * gym_lmaze/envs/lmaze_env.py, "vK" means gym_lmaze/envs/lmaze_env_vK.py.
 *
 * Conventions
 *   - plain pointers and sizes only; all pointers are DEVICE pointers (HBM) unless
 *     the name ends in _host; the caller owns every buffer; nothing is allocated,
 *     freed or synchronised inside; work is queued on `stream` (a hipStream_t passed
 *     as void*, NULL = the null stream).
 *   - N independent mazes ("envs"), struct-of-arrays, one element per env.
 *   - a maze layout is G*G bytes, row-major, holding the reference's own cell
 *     characters: 'W' wall, 'B' blank, 'S' start, 'X' goal marker (v0:37-48).
 *   - coordinates: x = row (first array axis), y = column, exactly as in the reference.
 *   - return value: 0 on success, a negative LMAZE_E_* for a rejected argument, or a
 *     positive hipError_t from the launch.
 */
#ifndef LMAZE_H_
#define LMAZE_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LMAZE_ABI_VERSION 4

/* which reference class the transition rules come from */
enum {
    LMAZE_VARIANT_V0 = 0, /* LmazeEnv      (v0:146-237) 4-neighbour, sticky reward           */
    LMAZE_VARIANT_V3 = 3  /* LmazeEnv_v3   (v3:220-402) 4-neighbour, look-ahead goal test    */
};

/* how `layout` is addressed */
enum {
    LMAZE_LAYOUT_SHARED = 0, /* one layout  uint8[G*G]    for every env (staged in LDS)      */
    LMAZE_LAYOUT_PER_ENV = 1 /* own layout  uint8[N*G*G]  per env (LDS tile per workgroup)   */
};

/* compact observation: one int32 per cell; every reference plane is a bit test */
enum {
    LMAZE_OBS_BALL = 1, /* v0 plane 0 (v0:80,178-183)  | v3 plane 1 (v3:167,256-261)         */
    LMAZE_OBS_WALL = 2, /* v0 plane 1 (v0:92-94): cell == 'W'                                */
    LMAZE_OBS_GOAL = 4, /* v0 plane 2 (v0:96-98): cell == 'X' | v3 plane 2: one-hot goal_xy  */
    LMAZE_OBS_FREE = 8  /* v0 plane 3 (v0:105-107): cell == 'B' | v3 plane 0: cell != 'W'    */
};

enum {
    LMAZE_E_NULL = -1,      /* a required pointer is NULL                                     */
    LMAZE_E_GRID = -2,      /* grid outside [3, LMAZE_MAX_GRID]                               */
    LMAZE_E_VARIANT = -3,   /* params.variant does not match the entry point                  */
    LMAZE_E_LAYOUT = -4,    /* unknown layout_mode                                            */
    LMAZE_E_COUNT = -5,     /* n < 0 or n too large for one launch                            */
    LMAZE_E_ALIGN = -6,     /* obs/ball_xy not aligned as documented                          */
    LMAZE_E_EXPANSION = -7, /* expansion ratio / channel count out of range                   */
    LMAZE_E_NODEVICE = -8   /* no HIP device / wrong architecture                             */
};

#define LMAZE_MAX_GRID 64
/* most envs one call accepts (LMAZE_E_COUNT beyond).  A launch is further limited to 2^24 - 1 workgroups of 256
 * threads (HIP: grid * block < 2^32); a count whose launch would need more -- the per-env-layout kernels take 4
 * envs per workgroup, i.e. 2^26 envs -- is refused with hipErrorInvalidConfiguration, never truncated. */
#define LMAZE_MAX_ENVS ((int64_t)1 << 30)
#define LMAZE_MAX_CHANNELS 8

/* Constants the reference hard-codes in __init__ (v0:17-23, v3:76-99). */
typedef struct LmazeParams {
    int32_t variant;     /* LMAZE_VARIANT_*                                                  */
    int32_t grid;        /* G = realgrid, side of the square layout incl. border (v0:17)     */
    int32_t layout_mode; /* LMAZE_LAYOUT_*                                                   */
    int32_t step_limit;  /* v0: done when stepCount == limit (v0:247); v3: > limit (v3:398)  */
    float reward_wall;   /* negativeNominal  -1.0   (v0:21)                                  */
    float reward_move;   /* positiveNominal  -0.01  (v0:22)                                  */
    float reward_goal;   /* positiveFull    100.0   (v0:23)                                  */
    int32_t launch_hint; /* 0 = library default launch policy.  Performance only, never results
                            (lmaze_step.hip step_plan); bits not listed are 0.              
                              bits 0-3   workgroups resident per CU (1..8; 0 = default)
                              bits 4-7   chunks of envs a workgroup takes one after the other, loading
                                         the next chunk's inputs while it stores the current one
                                         (1..15; 0 = default)
                              bit  8     keep the workgroup/LDS kernel where the library would pick the
                                         wave-autonomous one (8x8 shared layouts whose planes stay
                                         on-die); for the wave-autonomous kernel bits 4-7 = envs per
                                         wave (1: 64, 2: 32, 3: 16), bits 0-3 = waves per workgroup
                                         (1, 2, 4)
                              bit  9     streaming regime without the fused reset: drop the early wait on the
                                         per-env loads that staggers the workgroups of a CU (a measured +8-15 %
                                         at 1M x 11x11; the launch-policy guard test times both)
                              bits 10-11 envs per workgroup (0 = default):
                                           11x11, 12x12        1: 64   2: 32   3: 16
                                           14x14, 18x18        1: 32   2: 16
                                           8x8 (large batch)   1: 128  2: 64
                                           32x32               1: 8    2: 4
                                           any other G         1: 256  2: 64   3: 16                     */
} LmazeParams;

int lmaze_abi_version(void);

/* Human-readable text for a code returned by any entry point (static storage). */
const char* lmaze_strerror(int code);

/* Number of visible HIP devices and, for `device`, CU count / arch name ("gfx950").
 * Returns 0 or LMAZE_E_NODEVICE.  name_host may be NULL. */
int lmaze_device_info(int device, int32_t* cu_count_host, char* name_host, int32_t name_len);

/*
 * Which kernel, grid and launch policy lmaze_step_v0 / _v3 (auto_reset != 0: the *_autoreset forms) would queue for n
 * envs with these params -- decided by the very code that launches, nothing is queued or dereferenced.  text_host
 * receives one line, e.g. "step_shared_kernel<11, v0, step, 32, nt> grid=32768 block=256 lds=20480
 * envs_per_workgroup=32 workgroups_per_cu=0 chunks=1" (workgroups_per_cu 0 = no cap; with_obs: 0 transition only, 1 the
 * int32 planes, 2 the narrow planes of lmaze_step_u8).  For bench.py's
 * roofline.kernel and the launch-policy guard test; no reference counterpart.
 */
int lmaze_describe_step(const LmazeParams* params, int64_t n, int32_t auto_reset, int32_t with_obs, char* text_host,
                        int32_t len);

/*
 * LOADED STATE -- what lmaze_step_v0 / _v3 (and their *_autoreset and _u8 forms), lmaze_observe / _observe_u8, lmaze_reset
 * and every lmaze_rollout* entry do with per-env state that no reset produced.  The reference indexes its layout with the
 * coordinates as they are (v0:172, v3:251) and raises or wraps once they leave the grid; here nothing is read out of
 * bounds, by these rules, on layouts with a full 'W' border:
 *   - a step takes the ball clamped to 0..G-1 on each axis, and the target cell (ball + offset) clamped likewise; the
 *     ball it stores is the clamped one, moved or not.  That is the reference's own step on the maze with one more ring
 *     of 'W' around it: a ball on a border cell bumps when it walks outwards and moves when the cell inwards is free;
 *   - an observe-only launch shows the ball at its clamped cell and leaves ball_xy as loaded;
 *   - the v3 goal is compared as it is (v3:264, with the unclamped cell beyond the ball's new one) and gets its plane bit
 *     only when it lies on the grid; the closed-loop keys, and only they, clamp it;
 *   - done on entry (the fused reset's flag, a reset's mask) is set by any non-zero byte; a step stores 0 or 1;
 *   - a reset with no accepted cell leaves ball_xy and goal_xy untouched -- a fresh env on such a maze keeps its ball at
 *     (0, 0), a border cell, which the rules above cover -- and still zeroes step_count, reward and done; a v3 reset with
 *     one accepted cell places the goal there and leaves the ball; with more, the ball's draw skips the goal's cell;
 *   - a v0 reward that passes through a sticky pair (the target is 'S': v0:172-195 has no else) keeps its 32 bits,
 *     whatever they are -- a NaN's payload, a signalling NaN, -0.0, a denormal -- in the state and in the reward_t rows;
 *   - step_count is incremented as it is, from any value (a negative count, or one past the limit: v0's `==` then never
 *     fires again, v3's `>` fires every step).
 * tests/loaded_state.py holds these against the reference's own step on the padded maze.
 */

/*
 * One step() of N v0 mazes: replaces v0:146-237 (action decode 153-170, collision and
 * position update 172-195, reward 174/184/194, done 246-249, plane build 208-215).
 *   action      int32[N]    0:(-1,0) 1:(+1,0) 2:(0,-1) 3:(0,+1), anything else (0,0)
 *   ball_xy     int32[N,2]  (ball_x0, ball_y0), read and updated; 8-byte aligned
 *   step_count  int32[N]    stepCount, incremented first (v0:151)
 *   reward      float[N]    read AND written: v0 keeps the previous reward when the
 *                           target cell is neither 'W','B' nor 'X' (no else, v0:172-195)
 *   done        uint8[N]    reward == reward_goal || step_count == step_limit (v0:246-249)
 *   goal_count  int32[N]    goalCount (v0:195); may be NULL
 *   obs         int32[N,G,G] compact planes after the move, fully rewritten; may be NULL
 *                           (transition only); 16-byte aligned
 * Envs never auto-reset (the reference does not); stepping after done follows v0 exactly.
 * Coordinates off the grid, and any other state no reset produced: LOADED STATE above (lmaze_step_v3 alike).
 */
int lmaze_step_v0(const LmazeParams* params, const uint8_t* layout, const int32_t* action,
                  int32_t* ball_xy, int32_t* step_count, float* reward, uint8_t* done,
                  int32_t* goal_count, int32_t* obs, int64_t n, void* stream);

/*
 * One step() of N v3 mazes: replaces v3:220-402 (decode 234-247, collision/move 251-262,
 * look-ahead goal test 264-265, done 398).  The caller maps the reference's string
 * actions to ids ("left"/"0"->0, "right"/"1"->1, "up"/"2"->2, "down"/"3"->3, anything
 * else, including a Python int, -> a no-op id such as -1).
 *   goal_xy     int32[N,2]  (goal_x, goal_y), read only (set by reset, v3:147-152)
 *   reward      float[N]    written only (re-zeroed to -0.0 every step, v3:224)
 *   done        uint8[N]    reward == reward_goal || step_count > step_limit
 */
int lmaze_step_v3(const LmazeParams* params, const uint8_t* layout, const int32_t* action,
                  int32_t* ball_xy, const int32_t* goal_xy, int32_t* step_count, float* reward,
                  uint8_t* done, int32_t* obs, int64_t n, void* stream);

/*
 * Compact planes of the CURRENT state without stepping: what reset() returns after
 * placement (v0:92-120, v3:166-196).  goal_xy is read for LMAZE_VARIANT_V3 only (NULL
 * otherwise).  A ball off the grid is shown at its clamped cell and ball_xy is not written; a v3 goal
 * off the grid has no plane bit (LOADED STATE above).
 */
int lmaze_observe(const LmazeParams* params, const uint8_t* layout, const int32_t* ball_xy,
                  const int32_t* goal_xy, int32_t* obs, int64_t n, void* stream);

/*
 * Masked on-device reset: replaces the placement + bookkeeping part of reset()
 * (v0:67-110; v3:142-167).  For every env with mask[i] != 0 (mask NULL = all):
 * step_count = 0, reward = -0.0, done = 0, and a new ball cell (v3: first a new goal
 * cell) drawn uniformly from the cells the reference's rejection loop accepts
 * (v0:70-78: interior, not 'W', not 'X'; v3:147-161: goal interior not 'W', ball interior
 * not 'W' and != goal).  Draws come from Philox4x32-10 keyed by (seed, env_base + i,
 * epoch): env_base is the global index of this shard's env 0, so a batch sharded over
 * several GPUs draws exactly what one GPU holding the whole batch would.  The reference
 * draws from Python's global Mersenne Twister, so placement parity with it is
 * distributional, not bitwise.  obs (nullable): the planes of the envs that were reset are
 * re-rendered (with a mask, envs outside it keep their current planes: the planes are written in
 * 16-byte stores, and a store -- at odd G of the specialised sizes, a group of four envs -- that holds cells
 * of a reset env rewrites the cells of its neighbours too, from their unchanged state.  Planes that were
 * current stay what they were; stale ones, after steps without obs, may come back partly fresh).
 * A maze with no accepted cell: the coordinates stay as they are (the counters are still zeroed); a v3 maze
 * with one: the goal goes there and the ball stays; the render clamps a ball it finds off the grid (LOADED
 * STATE above).
 */
int lmaze_reset(const LmazeParams* params, const uint8_t* layout, const uint8_t* mask,
                uint64_t seed, uint64_t epoch, int64_t env_base, int32_t* ball_xy, int32_t* goal_xy,
                int32_t* step_count, float* reward, uint8_t* done, int32_t* obs, int64_t n,
                void* stream);

/*
 * lmaze_reset with the ball drawn from a start law the caller gives -- curricula over the distance field (start lo..hi
 * steps from the goal: lmaze_score's `optimal`), prioritised starts -- per problem, from the env's own reset draw, in one
 * placement launch.  No reference counterpart.  Below S = G*G and r = the reset draw of env i, Philox4x32-10 with
 * lmaze_reset's counter (env_base + i, epoch) and key (seed).  For every env with mask[i] != 0 (mask NULL = all):
 *   1. goal (v3 only)   keep_goal == 0: re-drawn exactly as lmaze_reset draws it, the ((r.x * count) >> 32)-th accepted cell
 *                       in row-major order, and with count == 0 it stays; keep_goal != 0: goal_xy[i] is left as it is.
 *                       v0 has no per-env goal.
 *   2. row              row_mode 0: row 0 of thresholds uint32[S], one law for every env;
 *                       row_mode 1: row i, the env's LOCAL index (not env_base + i), of uint32[n, S];
 *                       row_mode 2: v3 only, row clamp(goal_x) * G + clamp(goal_y) of uint32[S, S], the goal read AFTER 1.
 *   3. ball             u = r.y >> 1, a 31-bit draw, and k = #{ j in [0, S) : row[j] <= u }.  k < S: ball_xy[i] =
 *                       (k / G, k % G); k == S: the ball stays where it is, lmaze_reset's "no accepted cell" case.
 *   4. bookkeeping      step_count = 0, reward = -0.0, done = 0; obs (nullable): the masked re-render lmaze_reset queues.
 * A row is a cumulative law in units of 2^-31: cell j is drawn with probability (row[j] - row[j-1]) / 2^31, row[-1] = 0, and
 * a complete row ends in exactly 2^31.  (31 bits and not the sampling rollouts' 32 because 2^31 fits the word: zero-mass
 * cells behind the last massive one are never reached, where a 32-bit table would let one draw in 2^32 through to cell
 * S - 1, a border wall.)  A row of zeros is the "ball stays" row; a row of 2^31 everywhere puts the ball on cell 0.
 * Rows are expected non-decreasing; for those the binary search some forms run gives k.  The table is NOT read to validate
 * it: for any other row the result is some k in [0, S], and nothing is read or written out of bounds.  A cell is not
 * excluded for being a wall, an 'X' or the goal: what a step does with such a state is LOADED STATE above.
 *   thresholds  4-byte aligned device memory, read only; never written.
 * Refused before anything is queued, in this order: lmaze_reset's own refusals (the params, the variant, then LMAZE_E_NULL /
 * LMAZE_E_ALIGN for its buffers); LMAZE_E_COUNT row_mode outside {0, 1, 2}; LMAZE_E_VARIANT row_mode 2 or keep_goal != 0
 * on v0; LMAZE_E_NULL thresholds; LMAZE_E_ALIGN thresholds not 4-byte aligned.  n == 0 then returns 0 with nothing read.
 * Kernels: a shared layout with row_mode 0 or 2 -- one lane per env; the workgroup stages the one row in LDS (<= 16 KiB) or
 * reads the goal's row from global memory, a branch-free binary search of ceil(log2(S + 1)) probes; the v3 goal from the
 * workgroup's spawn list.  row_mode 1, and every row mode on per-env layouts -- one wave per env reads the S words
 * coalesced and sums the ballots of the compares; the v3 goal is ranked on the env's own layout.
 * Out of scope: the fused resets inside the *_autoreset steps and the one-launch rollouts keep lmaze_reset's uniform law (a
 * curriculum runs them without auto-reset and resets done envs between launches); the foveal envs; captured graphs (no
 * device-resident epoch here); compact threshold formats.
 */
int lmaze_reset_start(const LmazeParams* params, const uint8_t* layout, const uint8_t* mask, const uint32_t* thresholds,
                      int32_t row_mode, int32_t keep_goal, uint64_t seed, uint64_t epoch, int64_t env_base,
                      int32_t* ball_xy, int32_t* goal_xy, int32_t* step_count, float* reward, uint8_t* done, int32_t* obs,
                      int64_t n, void* stream);

/*
 * What lmaze_reset_start would queue for n envs, as lmaze_describe_step: "reset_start_kernel<v3, rows=goal, table=global>
 * grid=... block=256 lds=... envs_per_workgroup=256 workgroups_per_cu=0 chunks=1"; rows=one with table=lds on a shared
 * layout; rows=env, and every form on per-env layouts, table=global with envs_per_workgroup=4 (a wave per env).  Refusals:
 * the params and the variant, LMAZE_E_COUNT / LMAZE_E_VARIANT for row_mode as above, LMAZE_E_NULL for the text; n == 0
 * gives an empty line.
 */
int lmaze_describe_reset_start(const LmazeParams* params, int64_t n, int32_t row_mode, char* text_host, int32_t len);

/*
 * step() with the reset fused in front of it, for rollouts longer than one episode: an env
 * whose done[i] is set ON ENTRY (by the previous step) is first reset exactly as
 * lmaze_reset(mask = done, seed, epoch, env_base) would -- new placement, step_count = 0,
 * reward = -0.0 (v0:64-110, v3:134-167) -- and then takes this step's action, i.e. the
 * user loop `if done: env.reset()` followed by `env.step(a)`, in one launch and with no
 * extra HBM traffic.  Results are bit-identical to calling lmaze_reset then lmaze_step_*.
 * The caller advances `epoch` every call so successive episodes draw fresh placements.
 * goal_xy (v3) is read and, for reset envs, rewritten.
 *
 * Device-resident epoch (both nullable; for launches captured in a hipGraph, whose host
 * arguments are frozen): with epoch_in_dev != NULL the launch draws with epoch + *epoch_in_dev,
 * and with epoch_out_dev != NULL too its first workgroup stores *epoch_in_dev + 1 there.  The two
 * must be DIFFERENT 8-byte-aligned device words (the rest of the grid still reads the first);
 * a captured rollout alternates them launch by launch, so each replay continues the count and
 * draws fresh placements.  LMAZE_E_ALIGN if they alias, are misaligned, or only _out is given.
 */
int lmaze_step_v0_autoreset(const LmazeParams* params, const uint8_t* layout, const int32_t* action,
                            int32_t* ball_xy, int32_t* step_count, float* reward, uint8_t* done,
                            int32_t* goal_count, int32_t* obs, int64_t n, uint64_t seed,
                            uint64_t epoch, int64_t env_base, const uint64_t* epoch_in_dev,
                            uint64_t* epoch_out_dev, void* stream);

int lmaze_step_v3_autoreset(const LmazeParams* params, const uint8_t* layout, const int32_t* action,
                            int32_t* ball_xy, int32_t* goal_xy, int32_t* step_count, float* reward,
                            uint8_t* done, int32_t* obs, int64_t n, uint64_t seed, uint64_t epoch,
                            int64_t env_base, const uint64_t* epoch_in_dev, uint64_t* epoch_out_dev,
                            void* stream);

/*
 * The step with a NARROW observation: the same LMAZE_OBS_* bit mask in one byte per cell, obs8 uint8[N,G,G] (16-byte
 * aligned, nullable), 37 + G*G bytes per env-step instead of 37 + 4 G*G.  Shared layouts only (LMAZE_E_LAYOUT
 * otherwise); params->variant selects the rules, goal_xy is v3's (read; rewritten for reset envs), goal_count v0's (nullable).
 * auto_reset != 0 fuses the reset in exactly as lmaze_step_*_autoreset (seed, epoch, env_base, device-resident epoch words).
 * State and obs8 are what lmaze_step_v0 / _v3 leave, each plane dword narrowed to a byte.  The int32 planes remain the mode
 * BASELINE's metric is quoted on; this one has its own algorithmic bytes (bench.py --obs-dtype u8).
 * lmaze_observe_u8: the planes of the current state without stepping (mask != NULL: only the envs with mask[i] != 0).
 */
int lmaze_step_u8(const LmazeParams* params, const uint8_t* layout, const int32_t* action, int32_t* ball_xy, int32_t* goal_xy,
                  int32_t* step_count, float* reward, uint8_t* done, int32_t* goal_count, uint8_t* obs8, int64_t n,
                  int32_t auto_reset, uint64_t seed, uint64_t epoch, int64_t env_base, const uint64_t* epoch_in_dev,
                  uint64_t* epoch_out_dev, void* stream);
int lmaze_observe_u8(const LmazeParams* params, const uint8_t* layout, const int32_t* ball_xy, const int32_t* goal_xy,
                     const uint8_t* mask, uint8_t* obs8, int64_t n, void* stream);

/*
 * T steps of N v0 / v3 mazes over a pre-generated action tensor int32[T,N] (row t = step t): exactly T calls of
 * lmaze_step_v0 / _v3 -- with auto_reset != 0 of the *_autoreset forms, step t drawing with epoch + t -- with
 * bit-identical state and planes at the end (params->variant selects the rules; goal_xy for v3 only, goal_count for v0
 * only, both nullable as in the step calls).  reward_t float[T,N] / done_t uint8[T,N] (nullable) receive every step's
 * reward and done row.  The whole rollout is ONE launch: the lane that owns an env keeps its state in registers across the
 * T steps (on-die shared 8x8: a wave per 64 envs; otherwise a workgroup per 4-64 envs with the layout -- or its envs' own
 * layouts -- in LDS, read once per rollout), the planes are rewritten every step as T launches would, the per-env state
 * goes back once at the end (65 536 x 8x8: a step costs 6 us as a launch of its own, a third of it launch gap, 2.3-2.5 us
 * here; 1M x 32x32 per-env layouts 838 -> 722 us per step; lmaze_describe_step names the step kernel, this call its
 * rollout form; params->launch_hint bits 12-14 = k > 0: 4 << (k - 1) envs per workgroup instead of the size the library
 * picks -- for batches beyond the L2s the largest that keeps the resident workgroups' planes inside them; with per-env
 * layouts at most 64, and halved until their layouts fit one workgroup's 160 KiB of LDS (G > 50: 32); performance only).
 * The caller advances its epoch by T.  State no reset produced enters every rollout entry point as it enters T step calls
 * (LOADED STATE above): the same clamps, the same "leave unchanged" placements, the same 32 reward bits in reward_t.
 * LMAZE_E_COUNT T < 0.  T == 0 or n == 0 (once params are valid) returns 0 with nothing read: no pointer is looked at.
 */
int lmaze_rollout(const LmazeParams* params, const uint8_t* layout, const int32_t* actions, int32_t T, int32_t* ball_xy,
                  int32_t* goal_xy, int32_t* step_count, float* reward, uint8_t* done, int32_t* goal_count, int32_t* obs,
                  float* reward_t, uint8_t* done_t, int64_t n, int32_t auto_reset, uint64_t seed, uint64_t epoch,
                  int64_t env_base, void* stream);

/*
 * lmaze_rollout that also RECORDS observations: every k-th step's planes go into the caller's obs_t, and a step that
 * fills no slot stores no planes at all.  Same arguments as lmaze_rollout, then:
 *   obs_t      int32[T / obs_every, N, G, G], 16-byte aligned, 64-bit offsets (1M x 11x11 is 484 MB per slot).  Slot j
 *              holds exactly what obs holds after step (j + 1) * obs_every - 1 of T step calls, fused resets included;
 *              the last T % obs_every steps are not recorded.
 *   obs_every  k >= 1; or 0: the final planes only (obs_t must then be NULL).
 * obs (nullable as in lmaze_rollout) still receives the planes after the last step and nothing before; final state, obs,
 * reward_t / done_t and the epoch the caller advances are bit-identical to lmaze_rollout.  One launch wherever
 * lmaze_rollout is one (the kernels' recording forms, e.g. "rollout_shared_kernel<v0, obs_t>"); the T-launch fallback
 * (T == 1, launch_hint bit 8) gives each step launch its slot, NULL (transition only) or obs.  launch_hint bit 15:
 * the other store policy for the slots (performance only).
 * Refused before anything is queued: LMAZE_E_COUNT obs_every < 0, or obs_t given with obs_every == 0; LMAZE_E_NULL
 * obs_t NULL while T / obs_every > 0; LMAZE_E_ALIGN obs_t not 16-byte aligned; then every refusal of lmaze_rollout.
 */
int lmaze_rollout_obs(const LmazeParams* params, const uint8_t* layout, const int32_t* actions, int32_t T, int32_t* ball_xy,
                      int32_t* goal_xy, int32_t* step_count, float* reward, uint8_t* done, int32_t* goal_count, int32_t* obs,
                      float* reward_t, uint8_t* done_t, int64_t n, int32_t auto_reset, uint64_t seed, uint64_t epoch,
                      int64_t env_base, int32_t* obs_t, int32_t obs_every, void* stream);

/*
 * lmaze_rollout with the NARROW planes of lmaze_step_u8: the arguments of lmaze_rollout with uint8_t* obs8 (uint8[N,G,G],
 * 16-byte aligned, nullable) in place of int32_t* obs.  Replaces T calls of lmaze_step_u8 (auto_reset != 0: its fused
 * reset, step t drawing with epoch + t) with bit-identical state, obs8 and per-step reward_t / done_t rows.  ONE launch
 * of rollout_shared_u8_kernel for any T >= 1 and any batch size: a workgroup owns 16-256 envs for the whole rollout, the
 * layout, its byte-shifted plane patterns and the spawn list in LDS once, and rewrites obs8 every step as T step
 * launches would.  params->launch_hint bits 12-14 = k > 0: 4 << (k - 1) envs per workgroup (rounded up to 16, down to
 * what fits LDS) instead of the size the library picks; performance only.  The caller advances its epoch by T.
 * Refused before anything is queued: lmaze_step_u8's refusals (LMAZE_E_LAYOUT per-env layouts, LMAZE_E_GRID G < 4,
 * LMAZE_E_ALIGN obs8 not 16-byte aligned, ...) and LMAZE_E_COUNT T < 0; T == 0 or n == 0 (once params are valid)
 * returns 0 with nothing read.
 */
int lmaze_rollout_u8(const LmazeParams* params, const uint8_t* layout, const int32_t* actions, int32_t T, int32_t* ball_xy,
                     int32_t* goal_xy, int32_t* step_count, float* reward, uint8_t* done, int32_t* goal_count, uint8_t* obs8,
                     float* reward_t, uint8_t* done_t, int64_t n, int32_t auto_reset, uint64_t seed, uint64_t epoch,
                     int64_t env_base, void* stream);

/*
 * lmaze_rollout_obs for the narrow planes: replaces the T lmaze_step_u8 calls that recorded a u8 env's observations
 * (each writing its slot or nothing), in one launch.  Same arguments and obs_every semantics as lmaze_rollout_obs, with
 *   obs_t8     uint8[T / obs_every, N, G, G]; slot 0 16-byte aligned, slot j starts j N G G bytes further, at any byte
 *              offset (N = 777 at 11x11: 5 past a 16-byte boundary); no byte outside the slots is written.
 * obs8 receives the planes after the last step and nothing before.  Refused before anything is queued: LMAZE_E_COUNT
 * obs_every < 0, or obs_t8 given with obs_every == 0; LMAZE_E_NULL obs_t8 NULL while T / obs_every > 0; LMAZE_E_ALIGN
 * obs_t8 not 16-byte aligned; then every refusal of lmaze_rollout_u8, with T == 0 or n == 0 returning 0.
 */
int lmaze_rollout_obs_u8(const LmazeParams* params, const uint8_t* layout, const int32_t* actions, int32_t T, int32_t* ball_xy,
                         int32_t* goal_xy, int32_t* step_count, float* reward, uint8_t* done, int32_t* goal_count, uint8_t* obs8,
                         float* reward_t, uint8_t* done_t, int64_t n, int32_t auto_reset, uint64_t seed, uint64_t epoch,
                         int64_t env_base, uint8_t* obs_t8, int32_t obs_every, void* stream);

/*
 * As lmaze_describe_step, for the grid rollouts: which kernel, grid and envs per workgroup lmaze_rollout (with_obs 0:
 * obs NULL, 1: int32 obs) or lmaze_rollout_u8 (with_obs 2) would queue for n envs and T steps -- obs_every < 0 -- or
 * lmaze_rollout_obs / lmaze_rollout_obs_u8 with that obs_every (obs_t given when T / obs_every > 0), e.g.
 * "rollout_shared_kernel<v0> T=16 grid=1024 block=256 ...", "rollout_shared_u8_kernel<v3, obs_t> T=16 every=3 ...",
 * "rollout_perenv_kernel<v0, obs_t, nt> ..." (launch_hint bit 15: the slots' non-temporal stores), or the step kernel of
 * the T-launch fallback.  Nothing is queued or dereferenced; no reference counterpart.  T == 0 or
 * n == 0: an empty line.
 */
int lmaze_describe_rollout(const LmazeParams* params, int64_t n, int32_t T, int32_t auto_reset, int32_t with_obs,
                           int32_t obs_every, char* text_host, int32_t len);

/*
 * CLOSED-LOOP rollout: lmaze_rollout_obs with a tabular epsilon-greedy policy inside the kernel instead of a pre-generated
 * action tensor.  Replaces the user loop of T x (look the action up by the ball's cell, mix in exploration, step(): v0:146-237,
 * v3:220-402, with auto_reset != 0 the reset() of done envs first, v0:64-110) -- three or more launches per step -- by ONE
 * launch; the action selection itself has no reference counterpart.  The arguments of lmaze_rollout_obs with `actions`
 * replaced by
 *   policy       uint8[G^2] (key_mode 0) or uint8[G^4] (key_mode 1): the greedy action id of every key, passed through
 *                unchanged -- ids above 3 mean what they mean to lmaze_step_* (no move), nothing is validated
 *   key_mode     0: key = ball_x * G + ball_y (the row-major ball cell; v0 and v3, shared and per-env layouts);
 *                1: key = (goal_x * G + goal_y) * G^2 + ball cell (v3 only)
 *   epsilon_u32  min(floor(eps * 2^32), 2^32 - 1) for eps in [0, 1], computed by the caller; 0: nothing is drawn
 * and, beside reward_t / done_t,
 *   actions_t    int32[T,N], nullable: the action step t took
 *   key_t        int32[T,N], nullable: the key it was looked up with
 * Env i (global index e = env_base + i) at step t, ep = epoch + t:
 *   1. auto_reset != 0 and the env done: the fused reset exactly as lmaze_rollout's, same draw, same epoch ep;
 *   2. key of the state after that reset (coordinates as the transition takes them: clamped onto the grid);
 *   3. action = policy[key]; if epsilon_u32 != 0, r = Philox4x32-10(counter (e_lo, e_hi, ep_lo, ep_hi ^ 0x80000000), key
 *      (seed_lo, seed_hi)) and the action is r.y >> 30 when r.x < epsilon_u32.  The flipped top bit keeps this stream apart
 *      from the reset draw of the same (e, ep): callers keep epoch + T below 2^63;
 *   4. the transition of lmaze_step_v0 / _v3 with that action.
 * obs_t / obs_every as in lmaze_rollout_obs (0: the final planes only); planes are stored on recorded steps and after the
 * last one, never otherwise.  Always ONE launch of a closed-loop kernel form ("rollout_shared_kernel<v0, policy=ball,
 * obs_t>", rollout_perenv_kernel for per-env layouts; on-die 8x8 too goes through rollout_shared_kernel): launch_hint bit 8,
 * the T-launch fallback, does not apply; bits 12-14 (envs per workgroup) and bit 15 behave as in lmaze_rollout_obs.  The
 * ball-keyed table is staged into LDS once per workgroup and counted where the envs per workgroup are fitted to LDS; the
 * goal-conditioned one is read from global memory, one byte per env-step (14 KB at G = 11, 1 MB at G = 32).  The caller
 * advances its epoch by T whether or not auto_reset is set: exploration consumes epochs too.
 * Refused before anything is queued, in this order: lmaze_rollout_obs's recording refusals (LMAZE_E_COUNT obs_every < 0
 * or obs_t with obs_every == 0, LMAZE_E_NULL obs_t missing, LMAZE_E_ALIGN obs_t); params, variant and LMAZE_E_COUNT T < 0
 * as lmaze_rollout; LMAZE_E_COUNT key_mode outside {0, 1}; LMAZE_E_VARIANT key_mode 1 on v0; then T == 0 or n == 0 returns
 * 0 with nothing read; LMAZE_E_NULL a required pointer, policy included; LMAZE_E_ALIGN as lmaze_rollout.
 */
int lmaze_rollout_policy(const LmazeParams* params, const uint8_t* layout, const uint8_t* policy, int32_t key_mode,
                         uint32_t epsilon_u32, int32_t T, int32_t* ball_xy, int32_t* goal_xy, int32_t* step_count, float* reward,
                         uint8_t* done, int32_t* goal_count, int32_t* obs, float* reward_t, uint8_t* done_t, int32_t* actions_t,
                         int32_t* key_t, int64_t n, int32_t auto_reset, uint64_t seed, uint64_t epoch, int64_t env_base,
                         int32_t* obs_t, int32_t obs_every, void* stream);

/*
 * lmaze_rollout_policy with the NARROW planes: replaces the same user loop around lmaze_step_u8 (v0:146-237, v3:220-402).
 * uint8_t* obs8 / obs_t8 as in lmaze_rollout_obs_u8, its byte-offset slot rule included (slot 0 16-byte aligned, slot j
 * j N G G bytes further); shared layouts and G >= 4 only.  One launch of rollout_shared_u8_kernel's closed-loop form;
 * launch_hint bit 8 is not read, bits 12-14 as in lmaze_rollout_u8 with the table counted in the LDS fit.  Refusals:
 * those of lmaze_rollout_obs_u8 (LMAZE_E_LAYOUT per-env layouts, LMAZE_E_GRID G < 4 after the params' own), then
 * lmaze_rollout_policy's, in its order.
 */
int lmaze_rollout_policy_u8(const LmazeParams* params, const uint8_t* layout, const uint8_t* policy, int32_t key_mode,
                            uint32_t epsilon_u32, int32_t T, int32_t* ball_xy, int32_t* goal_xy, int32_t* step_count, float* reward,
                            uint8_t* done, int32_t* goal_count, uint8_t* obs8, float* reward_t, uint8_t* done_t, int32_t* actions_t,
                            int32_t* key_t, int64_t n, int32_t auto_reset, uint64_t seed, uint64_t epoch, int64_t env_base,
                            uint8_t* obs_t8, int32_t obs_every, void* stream);

/*
 * As lmaze_describe_rollout, for the closed-loop rollouts: which kernel form, grid, LDS and envs per workgroup
 * lmaze_rollout_policy (with_obs 0: obs NULL, 1: int32 obs) or lmaze_rollout_policy_u8 (with_obs 2) would queue with that
 * obs_every >= 0 and key_mode, e.g. "rollout_perenv_kernel<v3, policy=goal, obs_t> T=16 every=3 grid=...".  Nothing is
 * queued or dereferenced; no reference counterpart.  The refusals that need no buffer are the calls' own; T == 0 or
 * n == 0: an empty line.
 */
int lmaze_describe_rollout_policy(const LmazeParams* params, int64_t n, int32_t T, int32_t auto_reset, int32_t with_obs,
                                  int32_t obs_every, int32_t key_mode, char* text_host, int32_t len);

/*
 * SAMPLING closed-loop rollout: lmaze_rollout_policy with a categorical table policy -- an action drawn from a per-key
 * distribution over the four actions -- in place of the epsilon-greedy one.  Replaces the user loop of T x (gather
 * probs[key], draw the action (a multinomial), step(): v0:146-237, v3:220-402, with auto_reset != 0 the reset() of done
 * envs first, v0:64-110) -- several launches per step -- by ONE launch; the action selection itself has no reference
 * counterpart.  The arguments of lmaze_rollout_policy with `policy, key_mode, epsilon_u32` replaced by
 *   thresholds   uint32[S, 4], 16 bytes per key and 16-byte aligned; S = G^2 for key_mode 0 and G^4 for key_mode 1, the
 *                keys of lmaze_rollout_policy.  Words 0-2 are the cumulative thresholds c0 <= c1 <= c2 of the key's row;
 *                word 3 is reserved: it is loaded with the rest, as one 128-bit read, and ignored
 *   key_mode     as lmaze_rollout_policy
 * The sampling rule.  Env i (global index e = env_base + i) at step t, ep = epoch + t:
 *   1. auto_reset != 0 and the env done: the fused reset exactly as lmaze_rollout's, same draw, same epoch ep;
 *   2. key of the state after that reset (coordinates clamped onto the grid), (c0, c1, c2) = thresholds[key];
 *   3. r = the .x word of lmaze_rollout_policy's exploration draw: Philox4x32-10(counter (e_lo, e_hi, ep_lo,
 *      ep_hi ^ 0x80000000), key (seed_lo, seed_hi)), the reset draw's counter with the top bit of its last word flipped;
 *      action = (r >= c0) + (r >= c1) + (r >= c2), unsigned compares.  Always in 0..3, drawn on every env-step;
 *   4. the transition of lmaze_step_v0 / _v3 with that action.
 * So action k has probability (c_k - c_(k-1)) / 2^32 with c_(-1) = 0 and c_3 = 2^32.  The table is not validated: a
 * non-monotone row still yields an action in 0..3 by that formula.  A cumulative probability of exactly 1 cannot be stored
 * (it would be 2^32): a converter stores 2^32 - 1, i.e. 1 - 2^-32, so a row (1, 0, 0, 0) takes action 0 except for the one
 * draw r = 0xFFFFFFFF in 2^32, which takes action 3; deterministic policies belong to lmaze_rollout_policy.  Converting
 * probabilities p0..p3 (float64): a0 = p0, a1 = a0 + p1, a2 = a1 + p2, s = a2 + p3,
 * c_k = min(floor(a_k / s * 2^32 + 0.5), 2^32 - 1).
 * actions_t / key_t / reward_t / done_t rows, obs_t / obs_every and the planes as in lmaze_rollout_policy.  Always ONE
 * launch of a sampling kernel form ("rollout_shared_kernel<v0, sample=ball, table=lds, obs_t>"): launch_hint bit 8 is not
 * read; bits 12-14 and bit 15 behave as in lmaze_rollout_policy.  Where the table lives is decided by rule: ball-keyed and
 * G <= 32 (at most 16 KiB) it is staged into LDS once per workgroup (table=lds) and counted where the envs per workgroup
 * are fitted to LDS; otherwise (goal-conditioned, or G > 32) every env-step makes one 16-byte read from global memory
 * (table=global) and no LDS is reserved for it.  The caller advances its epoch by T whether or not auto_reset is set:
 * every env-step consumes a draw.
 * Refusals: lmaze_rollout_policy's, in its order, with `thresholds` in the place of `policy`; LMAZE_E_ALIGN for a table
 * that is not 16-byte aligned joins the other alignment refusals.
 */
int lmaze_rollout_sample(const LmazeParams* params, const uint8_t* layout, const uint32_t* thresholds, int32_t key_mode, int32_t T,
                         int32_t* ball_xy, int32_t* goal_xy, int32_t* step_count, float* reward, uint8_t* done, int32_t* goal_count,
                         int32_t* obs, float* reward_t, uint8_t* done_t, int32_t* actions_t, int32_t* key_t, int64_t n,
                         int32_t auto_reset, uint64_t seed, uint64_t epoch, int64_t env_base, int32_t* obs_t, int32_t obs_every,
                         void* stream);

/*
 * lmaze_rollout_sample with the NARROW planes: replaces the same user loop around lmaze_step_u8 (v0:146-237, v3:220-402).
 * obs8 / obs_t8, shapes and refusals as lmaze_rollout_policy_u8, then lmaze_rollout_sample's; one launch of
 * rollout_shared_u8_kernel's sampling form, the staged table counted in its 64-KiB LDS fit.  The epoch advances by T.
 */
int lmaze_rollout_sample_u8(const LmazeParams* params, const uint8_t* layout, const uint32_t* thresholds, int32_t key_mode, int32_t T,
                            int32_t* ball_xy, int32_t* goal_xy, int32_t* step_count, float* reward, uint8_t* done,
                            int32_t* goal_count, uint8_t* obs8, float* reward_t, uint8_t* done_t, int32_t* actions_t, int32_t* key_t,
                            int64_t n, int32_t auto_reset, uint64_t seed, uint64_t epoch, int64_t env_base, uint8_t* obs_t8,
                            int32_t obs_every, void* stream);

/*
 * As lmaze_describe_rollout_policy, for the sampling rollouts, e.g. "rollout_shared_kernel<v0, sample=ball, table=lds,
 * obs_t> T=16 every=3 grid=..."; table=global where the thresholds are read from global memory.  Nothing is queued or
 * dereferenced; no reference counterpart.
 */
int lmaze_describe_rollout_sample(const LmazeParams* params, int64_t n, int32_t T, int32_t auto_reset, int32_t with_obs,
                                  int32_t obs_every, int32_t key_mode, char* text_host, int32_t len);

/*
 * CLOSED-LOOP rollout with a table PER ENV: lmaze_rollout_policy with a third key rule, the one that runs what lmaze_solve
 * returns for per-env layouts (policy uint8[N, G^2]) or a population of policies on one shared maze.  Replaces the user loop
 * of T x (gather policy[i, ball cell], mix in exploration, step(): v0:146-237, v3:220-402, with auto_reset != 0 the reset()
 * of done envs first, v0:64-110) by ONE launch; the action selection itself has no reference counterpart.  The arguments of
 * lmaze_rollout_policy without key_mode, and
 *   policy       uint8[n * G^2], 4-byte aligned: row i * G^2 + c is the action id of env i at ball cell
 *                c = clamp(ball_x) * G + clamp(ball_y).  i is the LOCAL index 0 <= i < n of this call's buffers, not
 *                env_base + i: a shard passes its own envs' tables.  Ids above 3 are no move; nothing is validated
 *   key_t        int32[T,N], nullable: i * G^2 + c, the row the action was looked up in -- so values[key_t] gathers from a
 *                flat float32[n * G^2] table (lmaze_advantages_table) and lmaze_table_stats bins with keys = n * G^2
 * Everything else is lmaze_rollout_policy's to the bit: the fused reset and its draw, the exploration draw (counter word
 * ep_hi ^ 0x80000000, global env index e = env_base + i), r.y >> 30 when r.x < epsilon_u32, planes stored on recorded steps
 * and after the last one only, the caller's epoch advancing by T, always ONE launch (launch_hint bit 8 is not read; bits
 * 12-14 and bit 15 as in lmaze_rollout_obs).  int32 planes, v0 and v3, shared and per-env layouts.
 * v3: the table is keyed by the ball cell alone.  A fused reset re-draws the env's goal, so a table solved for the current
 * goal_xy is stale after it: pass auto_reset = 0, or tables that do not depend on the goal.  v0's goal is the layout's 'X'.
 * Where the table is read: per-env layouts ("rollout_perenv_kernel<v0, policy=env, table=lds, obs_t>") stage the workgroup's
 * envs_per_workgroup * G^2 table bytes into LDS once, behind its layouts -- counted where the envs per workgroup are clamped
 * to LDS --; shared layouts ("rollout_shared_kernel<v0, policy=env, table=global>") read one byte per env-step from global
 * memory.
 * Refusals: lmaze_rollout_policy's, in its order, with this in the place of the key mode's: LMAZE_E_COUNT when
 * n * G^2 > INT32_MAX (refused whether or not key_t is given, and before T == 0 or n == 0 returns 0 with nothing read, not even
 * an alignment); LMAZE_E_ALIGN for a policy that is not 4-byte aligned joins the other alignment refusals.
 */
int lmaze_env_rollout_policy(const LmazeParams* params, const uint8_t* layout, const uint8_t* policy, uint32_t epsilon_u32,
                             int32_t T, int32_t* ball_xy, int32_t* goal_xy, int32_t* step_count, float* reward, uint8_t* done,
                             int32_t* goal_count, int32_t* obs, float* reward_t, uint8_t* done_t, int32_t* actions_t, int32_t* key_t,
                             int64_t n, int32_t auto_reset, uint64_t seed, uint64_t epoch, int64_t env_base, int32_t* obs_t,
                             int32_t obs_every, void* stream);

/*
 * SAMPLING closed-loop rollout with a table PER ENV: lmaze_rollout_sample with lmaze_env_rollout_policy's key rule.  Replaces
 * the user loop of T x (gather probs[i, ball cell], draw the action, step(): v0:146-237, v3:220-402, with auto_reset != 0 the
 * reset() of done envs first, v0:64-110) by ONE launch; the action selection itself has no reference counterpart.  The
 * arguments of lmaze_rollout_sample without key_mode, and
 *   thresholds   uint32[n * G^2, 4], 16-byte aligned: row i * G^2 + c holds (c0, c1, c2, reserved) of env i (local index) at
 *                ball cell c; lmaze_rollout_sample's sampling rule, draw and conversion
 * key_t as in lmaze_env_rollout_policy, and its note on v3 and the fused reset.  Every env-step makes one 128-bit read of
 * its env's own row from global memory ("rollout_perenv_kernel<v3, sample=env, table=global>"): 16 bytes per cell and env do
 * not fit LDS beside the layouts, and none is reserved.
 * Refusals: lmaze_env_rollout_policy's, with LMAZE_E_ALIGN for thresholds that are not 16-byte aligned.
 */
int lmaze_env_rollout_sample(const LmazeParams* params, const uint8_t* layout, const uint32_t* thresholds, int32_t T,
                             int32_t* ball_xy, int32_t* goal_xy, int32_t* step_count, float* reward, uint8_t* done,
                             int32_t* goal_count, int32_t* obs, float* reward_t, uint8_t* done_t, int32_t* actions_t, int32_t* key_t,
                             int64_t n, int32_t auto_reset, uint64_t seed, uint64_t epoch, int64_t env_base, int32_t* obs_t,
                             int32_t obs_every, void* stream);

/*
 * As lmaze_describe_rollout_policy, for the rollouts with a table per env: form 0 lmaze_env_rollout_policy, 1
 * lmaze_env_rollout_sample; with_obs 0 (obs NULL) or 1 (int32 obs), e.g. "rollout_perenv_kernel<v0, policy=env, table=lds,
 * obs_t> T=16 every=3 grid=... lds=... envs_per_workgroup=..." or "rollout_shared_kernel<v3, sample=env, table=global> ...".
 * Nothing is queued or dereferenced; no reference counterpart.  LMAZE_E_COUNT for obs_every < 0, with_obs == 2 (there are
 * no narrow planes here) or a form outside {0, 1}; then the calls' own refusals that need no buffer; T == 0 or n == 0: an
 * empty line.
 */
int lmaze_describe_env_rollout(const LmazeParams* params, int64_t n, int32_t T, int32_t auto_reset, int32_t with_obs,
                               int32_t obs_every, int32_t form, char* text_host, int32_t len);

/*
 * Q-LEARNING inside the closed-loop rollout, a learner PER ENV: lmaze_env_rollout_policy acting on a table of action values
 * that the same launch updates after every transition.  Replaces the user loop of T x (gather q[i, ball cell], take the
 * maximum, mix in exploration, step(): v0:146-237, v3:220-402, with auto_reset != 0 the reset() of done envs first,
 * v0:64-110, gather the next row, take its maximum, scatter one update) by ONE launch; the learner itself has no reference
 * counterpart.  The arguments of lmaze_env_rollout_policy with q, alpha, gamma in the place of policy, and td_t:
 *   q            float32[n * G^2, 4], 16-byte aligned, UPDATED IN PLACE: row i * G^2 + c holds the four action values of env i
 *                (the LOCAL index 0 <= i < n, as lmaze_env_rollout_policy's) at ball cell c = clamp(ball_x) * G + clamp(ball_y)
 *   alpha, gamma the step size and the discount, float32; not validated (as lmaze_returns' gamma)
 *   td_t         float32[T,N], nullable, 4-byte aligned: the TD error of every step
 * Env i at step t, global index e = env_base + i, ep = epoch + t:
 *   1. the fused reset of a done env when auto_reset != 0: lmaze_env_rollout_policy's, same draw, same epoch;
 *   2. c as above, row = q[i * G^2 + c] (128 bits), greedy = the FIRST maximum of the row, by a strict > from action 0
 *      on -- lmaze_solve's rule; a NaN never wins, a row whose q[.., 0] is NaN keeps action 0;
 *   3. exploration as lmaze_rollout_policy's to the bit: epsilon_u32 == 0 draws nothing, else r = the policy draw of
 *      (seed, ep, e) and the action is r.y >> 30 when r.x < epsilon_u32; actions_t[t, i] and key_t[t, i] = i * G^2 + c;
 *   4. the transition of lmaze_step_v0 / _v3 with that action (sticky pairs, step limit and all);
 *   5. c' the ball cell after it, d the step's own done flag (the step limit counts), v_next = the first maximum of
 *      q[i * G^2 + c'] read BEFORE this step's write; target = reward when d, else reward + gamma * v_next (the product
 *      rounded, then the sum); delta = target - q[c, a]; q[c, a] = q[c, a] + alpha * delta (the product rounded, then the
 *      sum; never a fused multiply-add); td_t[t, i] = delta;
 *   6. reward_t / done_t rows and the planes as in the other closed-loop forms.
 * An env that enters a step done without auto_reset steps on as lmaze_step_* does and updates all the same.  Only env i's
 * own lane reads or writes its rows, so an env's updates are one sequential float32 recurrence, reproducible bit for bit
 * (csrc/lmaze_learn.h holds the arithmetic); the caller's epoch advances by T; always ONE launch (launch_hint bits 12-14 and
 * bit 15 as in lmaze_rollout_obs).  int32 planes, v0 and v3, shared and per-env layouts.
 * v3: the key is the ball cell alone and a fused reset re-draws the env's goal, so what v3 learns with auto_reset != 0 is
 * goal-free: values averaged over the goals drawn.  v0's goal is the layout's 'X' and does not move.
 * Where the table lives: global memory, the env's own rows read and written by its lane ("rollout_perenv_kernel<v0,
 * qlearn=env, table=global, obs_t>"): 16 bytes per cell and env do not fit LDS beside the layouts, and none is reserved.
 * The row read in 5 is the row of 2 at the next step unless a reset moves the ball; the lane keeps it in registers (on a
 * wall bump, c' == c, the row it has just written) and reads the table again only where the cells differ.
 * Refusals: lmaze_env_rollout_policy's, in its order, with q in the place of policy: LMAZE_E_COUNT when n * G^2 > INT32_MAX
 * (before T == 0 or n == 0 returns 0 with nothing read), LMAZE_E_NULL for a missing q, LMAZE_E_ALIGN for a q that is not
 * 16-byte aligned or a td_t that is not 4-byte aligned.
 */
int lmaze_env_rollout_qlearn(const LmazeParams* params, const uint8_t* layout, float* q, float alpha, float gamma,
                             uint32_t epsilon_u32, int32_t T, int32_t* ball_xy, int32_t* goal_xy, int32_t* step_count, float* reward,
                             uint8_t* done, int32_t* goal_count, int32_t* obs, float* reward_t, uint8_t* done_t, int32_t* actions_t,
                             int32_t* key_t, float* td_t, int64_t n, int32_t auto_reset, uint64_t seed, uint64_t epoch,
                             int64_t env_base, int32_t* obs_t, int32_t obs_every, void* stream);

/*
 * As lmaze_describe_env_rollout, for lmaze_env_rollout_qlearn (an entry of its own: lmaze_describe_env_rollout keeps its
 * forms 0 and 1), e.g. "rollout_perenv_kernel<v0, qlearn=env, table=global, obs_t> T=16 every=3 grid=... lds=...
 * envs_per_workgroup=...".  LMAZE_E_COUNT for obs_every < 0 or with_obs == 2; T == 0 or n == 0: an empty line.
 */
int lmaze_describe_env_rollout_qlearn(const LmazeParams* params, int64_t n, int32_t T, int32_t auto_reset, int32_t with_obs,
                                      int32_t obs_every, char* text_host, int32_t len);

/*
 * Discounted returns-to-go over the [T, N] rows a rollout writes; no reference counterpart (the reference keeps no
 * trajectories).  Replaces the T dependent steps of a host-driven reverse loop by ONE launch, one lane per env:
 *   ret = tail[i] (0 when tail is NULL); for t = T-1 .. 0:
 *   ret = reward_t[t, i] where done_t[t, i] != 0, else reward_t[t, i] + gamma * ret;  returns_t[t, i] = ret
 * in float32 with the product and the sum rounded separately (round to nearest even, never a fused multiply-add), so a
 * float32 loop on the host reproduces every bit.  reward_t float[T,N], done_t uint8[T,N], tail float[N] or NULL (the
 * value estimate behind the last row), returns_t float[T,N]; returns_t may be reward_t.  Refused: LMAZE_E_NULL reward_t,
 * done_t or returns_t missing; LMAZE_E_COUNT T < 0 or n outside [0, LMAZE_MAX_ENVS].  T == 0 or n == 0 returns 0 with
 * nothing read.
 */
int lmaze_returns(const float* reward_t, const uint8_t* done_t, const float* tail, float gamma, float* returns_t, int32_t T,
                  int64_t n, void* stream);

/*
 * Generalised advantage estimation, GAE(lambda), over the [T, N] rows a rollout writes, in ONE launch, one lane per env; no
 * reference counterpart.  Replaces the T dependent steps of a host-driven reverse loop.  With v(t, i) the value of row t and
 * v(T, i) the value behind the last row:
 *   gl = gamma * lambda (one float32 product, computed once);  v_next = v(T, i);  adv = 0;  for t = T-1 .. 0:
 *     v = v(t, i)
 *     adv = reward_t[t, i] - v                                      where done_t[t, i] != 0
 *     adv = ((reward_t[t, i] + gamma * v_next) - v) + gl * adv      otherwise
 *     adv_t[t, i] = adv;  target_t[t, i] = adv + v (when target_t is given);  v_next = v
 * in float32, every operation rounded on its own (round to nearest even, never a fused multiply-add), so a float32 loop on
 * the host reproduces every bit.  A done row cuts both the bootstrap and the trace, as in lmaze_returns: the done of a step
 * limit is treated as terminal like any other (the rows do not tell the two apart).
 *   lmaze_advantages        v(t, i) = value_t[t, i], value_t float[T,N];  v(T, i) = tail[i], tail float[N] or NULL (0).
 *   lmaze_advantages_table  v(t, i) = values[key_t[t, i]] where 0 <= key < keys and 0 otherwise (one unsigned compare, never
 *                           a read outside the table), key_t int32[T,N] as the closed-loop rollouts write it, values
 *                           float[keys];  v(T, i) the same lookup of key_tail[i], key_tail int32[N] or NULL (0).
 * reward_t float[T,N], done_t uint8[T,N], adv_t float[T,N], target_t float[T,N] or NULL.  adv_t may be reward_t, and in the
 * rows form target_t may be value_t: a lane reads a row of its own column before it stores it and touches no other column.
 * Refused, in this order: LMAZE_E_NULL reward_t, done_t, adv_t, value_t (rows form) or key_t / values (table form) missing;
 * LMAZE_E_COUNT T < 0, n outside [0, LMAZE_MAX_ENVS] or keys < 1.  T == 0 or n == 0 returns 0 with nothing read.
 */
int lmaze_advantages(const float* reward_t, const uint8_t* done_t, const float* value_t, const float* tail, float gamma,
                     float lambda, float* adv_t, float* target_t, int32_t T, int64_t n, void* stream);
int lmaze_advantages_table(const float* reward_t, const uint8_t* done_t, const int32_t* key_t, const int32_t* key_tail,
                           const float* values, int64_t keys, float gamma, float lambda, float* adv_t, float* target_t, int32_t T,
                           int64_t n, void* stream);

/*
 * Counts and sums per (key, action) over m samples -- the flattened [T, N] rows of a rollout -- bitwise reproducible; no
 * reference counterpart.  For sample j: bin = key_t[j] * actions + a, a = actions_t[j] (0 when actions_t is NULL, which
 * requires actions == 1).  A sample is skipped entirely -- neither counted nor summed -- when its key is outside [0, keys),
 * its action is outside [0, actions) (lmaze_rollout_policy writes ids above 3 for "no move"), or a weight row is given and
 * its weight is not finite or |w| >= 2^31.  Otherwise count[bin] += 1 and total_q24[bin] += q(w), where q(w) is w * 2^24
 * rounded to the nearest integer, ties to even: the product is exact in float32, so this is one rounding in all; on the
 * host, rint(double(w) * 2^24).  A mean is total_q24 / 2^24 / count.  Integer accumulation: the sums do not depend on the
 * order the samples arrive in, so any two runs, and the two kernels below, give the same 64 bits.
 *   key_t int32[m];  actions_t int32[m] or NULL;  weight_t float[m] and total_q24 int64[keys * actions], NULL together
 *   (counts only);  count int64[keys * actions].  Rows 4-byte aligned, tables 8-byte aligned (LMAZE_E_ALIGN).
 * The call adds onto what count / total_q24 hold -- the caller zeroes them -- so statistics can span several rollouts, and
 * several GPUs sum their tables exactly with one int64 all_reduce.  Range is the caller's: the sum of |w| per bin stays
 * below 2^39; beyond that the sum wraps, it never faults.
 * Where the table lives is a rule: up to 4096 bins (keys * actions <= 4096, every ball-keyed table up to G = 32) each
 * workgroup keeps a private table in LDS, 16 bytes per bin and sized to the table, accumulates into it with LDS atomics and
 * adds its non-zero bins to the global table with one 64-bit atomic each; above that, 64-bit global atomics per sample.
 * Always one launch.
 * Refused, in this order: LMAZE_E_NULL key_t or count missing; LMAZE_E_NULL exactly one of weight_t / total_q24 given;
 * LMAZE_E_COUNT m < 0, keys < 1, actions outside [1, 255], keys * actions > 2^28, or actions_t NULL with actions != 1.
 * m == 0 then returns 0 with nothing read.
 */
int lmaze_table_stats(const int32_t* key_t, const int32_t* actions_t, const float* weight_t, int64_t m, int64_t keys,
                      int32_t actions, int64_t* count, int64_t* total_q24, void* stream);

/*
 * The launch lmaze_table_stats would queue for these counts, one line in text_host (HOST, len bytes), e.g.
 * "table_stats_kernel<lds> grid=1024 block=256 lds=7744 bins=484", or "table_stats_kernel<global> ... lds=0 ...": written
 * by the code that launches, nothing queued or dereferenced.  An empty line for m == 0.  LMAZE_E_NULL text_host NULL or
 * len < 1, then lmaze_table_stats' LMAZE_E_COUNT refusals (actions != 1 stands for a given actions_t).
 */
int lmaze_describe_table_stats(int64_t m, int64_t keys, int32_t actions, char* text_host, int32_t len);

/*
 * The probability with which a table rule RECORDS the action of a row, for m samples -- the flattened [T, N] key_t and
 * actions_t rows of a closed-loop rollout -- in one launch, one lane per sample; no reference counterpart.  The table is
 * given in exactly one of lmaze_evaluate's three forms, `keys` rows of it, and a (key, action) pair weighs, in units of 2^-34:
 *   thresholds uint32[keys, 4]   the three words of row `key` in ascending order s0 <= s1 <= s2, s(-1) = 0, s3 = 2^32:
 *                                w = 4 (s_a - s_(a-1)) for a in 0..3 and 0 for any other id; word 3 is ignored;
 *   policy uint8[keys]           w = (0 <= a <= 3 ? epsilon_u32 : 0) + (a == policy[key] ? 4 (2^32 - epsilon_u32) : 0): a byte
 *                                above 3, recorded as the action, carries its greedy share;
 *   q float[keys, 4]             the same, the greedy action being the first maximum by a strict '>' (a NaN never wins,
 *                                nothing beats a NaN in word 0).
 * A key outside [0, keys) weighs 0 (one unsigned compare, never a read outside the table).  prob_t[j] = fl(w) * 2^-34: the
 * conversion rounds to nearest even and is the only rounding.  This is the law of the action the rollout records, with no
 * exclusion and no renormalisation -- not lmaze_evaluate's law, which is conditioned on the usable pairs.
 * key_t, actions_t int32[m], prob_t float[m].
 * Refused, in this order: LMAZE_E_NULL key_t, actions_t or prob_t missing; LMAZE_E_NULL unless exactly one of policy, q and
 * thresholds is given; LMAZE_E_COUNT m < 0 or keys < 1; LMAZE_E_ALIGN q or thresholds off 16 bytes, a row off 4.  m == 0 then
 * returns 0 with nothing read.
 */
int lmaze_action_probs(const int32_t* key_t, const int32_t* actions_t, int64_t m, const uint8_t* policy, const float* q,
                       uint32_t epsilon_u32, const uint32_t* thresholds, int64_t keys, float* prob_t, void* stream);

/*
 * V-trace (Espeholt et al. 2018: Retrace's lambda-return clipped at rho_bar and c_bar) over the [T, N] rows a rollout wrote
 * under a table that is no longer the one being learnt, in ONE launch, one lane per env; no reference counterpart.  With
 * v(t, i) the value of row t, v(T, i) the value behind the last row and ratio(t, i) the UNCLIPPED importance ratio of the row:
 *   v_next = vs_next = v(T, i);  acc_next = 0;  for t = T-1 .. 0, with r = reward_t[t, i], v = v(t, i), ratio = ratio(t, i):
 *     rho = ratio < rho_bar ? ratio : rho_bar;   cc = ratio < c_bar ? ratio : c_bar;   c = lambda * cc
 *     done_t[t, i] != 0:  td = r - v;                          acc = rho * td;                                  qv = r
 *     otherwise:          td = (r + gamma * v_next) - v;       acc = rho * td + (gamma * c) * acc_next;         qv = r + gamma * vs_next
 *     vs_t[t, i] = vs = acc + v;   pg_adv_t[t, i] = rho * (qv - v);   v_next = v;  vs_next = vs;  acc_next = acc
 * in float32, every operation rounded on its own in the order written (round to nearest even, never a fused multiply-add), so
 * a float32 loop on the host reproduces every bit.  A done row cuts the bootstrap and the trace, and the done of a step limit
 * is terminal like any other, as in lmaze_advantages.  A NaN ratio is clipped to the bars; gamma, lambda and the bars are not
 * validated.  On-policy (ratio 1, both bars >= 1) acc is lmaze_advantages' adv_t and vs its target_t in every bit.
 *   lmaze_vtrace        v(t, i) = value_t[t, i];  v(T, i) = tail[i], tail float[N] or NULL (0);  ratio(t, i) = rho_t[t, i],
 *                       rho_t float[T,N] or NULL (1).
 *   lmaze_vtrace_table  v by lmaze_advantages_table's rule from values float[keys], key_t int32[T,N] and key_tail int32[N] or
 *                       NULL (0);  ratio(t, i) = fl(fl(wt) / fl(wb)), wt and wb lmaze_action_probs' weights of
 *                       (key_t[t, i], actions_t[t, i]) under the target (t_*) and the behaviour (b_*) table, one correctly
 *                       rounded division, and 0 where wb == 0: a row the behaviour table cannot have produced carries no
 *                       weight.  Each table in exactly one of the three forms, `keys` rows; the forms need not match.  Equal
 *                       tables give exactly 1.  rho_out_t float[T,N] or NULL receives the unclipped ratio.
 * vs_t and pg_adv_t float[T,N], each may be NULL but not both.  Any output may be a float input row of the same call (a lane
 * reads the rows of its own column before it stores them and touches no other column); the outputs are distinct.
 * Refused, in this order: LMAZE_E_NULL reward_t, done_t, value_t (rows form) or key_t / actions_t / values (table form)
 * missing, or neither vs_t nor pg_adv_t given; LMAZE_E_NULL unless exactly one of policy, q and thresholds is given, for the
 * behaviour table, then for the target table; LMAZE_E_COUNT T < 0, n outside [0, LMAZE_MAX_ENVS] or keys < 1; LMAZE_E_ALIGN a q
 * or thresholds table off 16 bytes, a float or int32 pointer off 4.  T == 0 or n == 0 then returns 0 with nothing read.
 */
int lmaze_vtrace(const float* reward_t, const uint8_t* done_t, const float* value_t, const float* tail, const float* rho_t,
                 float gamma, float lambda, float rho_bar, float c_bar, float* vs_t, float* pg_adv_t, int32_t T, int64_t n,
                 void* stream);
int lmaze_vtrace_table(const float* reward_t, const uint8_t* done_t, const int32_t* key_t, const int32_t* actions_t,
                       const int32_t* key_tail, const float* values, int64_t keys, const uint8_t* b_policy, const float* b_q,
                       uint32_t b_epsilon_u32, const uint32_t* b_thresholds, const uint8_t* t_policy, const float* t_q,
                       uint32_t t_epsilon_u32, const uint32_t* t_thresholds, float gamma, float lambda, float rho_bar,
                       float c_bar, float* vs_t, float* pg_adv_t, float* rho_out_t, int32_t T, int64_t n, void* stream);

/*
 * VALUE ITERATION over the grid mazes: the optimal Q table of every maze, in ONE launch; no reference counterpart (the
 * reference has no planner).  It is the table lmaze_rollout_policy, lmaze_rollout_sample and lmaze_advantages_table take.
 * Problem p is one maze of S = G*G states, state s = x * G + y (the ball-cell key of the closed-loop rollouts), and the four
 * actions.  LMAZE_LAYOUT_SHARED: every problem reads layouts[0 .. G*G); LMAZE_LAYOUT_PER_ENV: problem p reads layouts + p*G*G.
 * v3 takes the goal of problem p from goal_xy[2p], goal_xy[2p+1], compared as it is (a goal off the grid is never hit); v0
 * does not read goal_xy, its goal is the layout's 'X'.
 * The model is the transition of lmaze_step_v0 / _v3 itself (v0:172-195, v0:246-249, v3:224-265, v3:398), asked once per
 * (cell, action) with a step count that trips no limit: the step limit is not part of the model, this is the
 * infinite-horizon discounted problem.  For a state on a non-wall cell, with c the character of the target cell:
 *   c == 'W'                 next = s, r = reward_wall
 *   v0, c == 'B' / 'X'       next = target, r = reward_move / reward_goal
 *   v3, any other c          next = target, r = reward_goal if the cell beyond the target is the goal, else reward_move
 *   a pair is terminal exactly when r == reward_goal as float32 (the step's own done rule: reward_wall == reward_goal makes a
 *   bump terminal)
 *   v0, any other c ('S')    a STICKY pair: the step leaves the ball where it is and repeats the previous reward, which is no
 *                            function of (cell, action).  Sticky pairs are excluded: q(s, a) = -INFINITY, never the maximum;
 *                            a state all of whose four pairs are excluded gets v = 0, policy = 0.  (lmaze_evaluate, which
 *                            takes an expectation where this takes a maximum, renormalises the mass a policy puts on
 *                            excluded pairs over the usable ones.)
 * A state on a 'W' cell has q = 0 for all four actions, v = 0, policy = 0.  Layouts carry a full 'W' border (every target of
 * a non-wall state is on the grid); on any other bytes a target off the grid counts as the cell itself, nothing is read out of
 * bounds.
 * The sweep is Jacobi, in float32, every operation rounded on its own (round to nearest even, never a fused multiply-add), as
 * lmaze_returns:
 *   V_0 = v_init (problem p: v_init + p*S) or 0 when v_init is NULL
 *   Q_k(s, a) = r(s, a) for a terminal pair, else r(s, a) + gamma * V_(k-1)(next)     (the product, then the sum)
 *   V_k(s) = the first maximum over a = 0, 1, 2, 3 by a strict '>' starting from a = 0; policy(s) = that a
 * Sweeps run until one leaves the bit pattern of every V(s) of the problem unchanged -- that sweep counts -- or until `sweeps`
 * have run; stopping early changes no output, the fixed point stays fixed.  Outputs, each nullable:
 *   q           float[problems, S, 4]  Q_k of the last executed sweep; 16-byte aligned
 *   v           float[problems, S]     V_k: max_a q bit for bit
 *   policy      uint8[problems, S]
 *   sweeps_run  int32[problems]        sweeps executed
 *   delta       float[problems]        max_s |V_k(s) - V_(k-1)(s)| of the last executed sweep, a maximum over the bit patterns
 *                                      of non-negative floats: it does not depend on the order of the reduction
 * One launch of solve_kernel: a problem lives in LDS for the whole solve (two V buffers; the model packed in registers); a wave
 * per problem while G*G <= 256, four problems per workgroup and no workgroup barrier; a workgroup per problem above, one
 * barrier per sweep.  params->launch_hint, step_limit are not read.
 * Refused, in this order: LMAZE_E_NULL params or layouts; LMAZE_E_GRID; LMAZE_E_VARIANT neither v0 nor v3; LMAZE_E_LAYOUT;
 * LMAZE_E_NULL goal_xy for v3; LMAZE_E_NULL all of q, v and policy; LMAZE_E_COUNT problems outside [0, LMAZE_MAX_ENVS] or
 * sweeps < 1; LMAZE_E_ALIGN q off 16 bytes, goal_xy (v3) off 8, a float or int32 pointer off 4.  problems == 0 then returns 0
 * with nothing read.  gamma is not validated, as in lmaze_returns.  A grid beyond 2^24 - 1 workgroups:
 * hipErrorInvalidConfiguration.
 */
int lmaze_solve(const LmazeParams* params, const uint8_t* layouts, const int32_t* goal_xy, int64_t problems, float gamma,
                int32_t sweeps, const float* v_init, float* q, float* v, uint8_t* policy, int32_t* sweeps_run, float* delta,
                void* stream);

/*
 * The launch lmaze_solve would queue, one line in text_host (HOST, len bytes), written by the code that launches, e.g.
 * "solve_kernel<v0, wave, 4> grid=65 block=256 lds=8192 problems_per_workgroup=4" or "solve_kernel<v3, workgroup, 2> ..."
 * (the third argument: cells per lane).  Nothing is queued or dereferenced.  LMAZE_E_NULL params or text_host NULL or
 * len < 1, then lmaze_solve's refusals of the params and of `problems`; an empty line for problems == 0.
 */
int lmaze_describe_solve(const LmazeParams* params, int64_t problems, char* text_host, int32_t len);

/*
 * SCORING TABLES on the grid mazes: from every cell, the fewest steps after which done can be set, and the number of steps
 * after which the walk that takes a table's action in every cell sets it, in ONE launch; no reference counterpart.  It tells
 * how good the tables are that lmaze_solve plans, lmaze_env_rollout_policy runs and lmaze_env_rollout_qlearn learns, exactly
 * and from every start cell at once: no rollout, no step limit, and a loop is told from a long path.
 * Problems and the model.  Problem p has S = G*G states, s = x * G + y.  Its model is lmaze_solve's, word for word: the
 * transition of lmaze_step_v0 / _v3 asked once per (cell, action) with a step count that trips no limit; the same wall, move
 * and goal pairs; a pair is terminal exactly when its reward equals reward_goal as float32; v0's sticky pairs are excluded;
 * wall states and targets off the grid as in lmaze_solve.  LMAZE_LAYOUT_SHARED: every problem reads the one layout and its own
 * table (a population of tables on one maze, v3 with one goal per problem, the goal-keyed tables); LMAZE_LAYOUT_PER_ENV: problem
 * p reads layouts + p*G*G.  v3 reads goal_xy[2p], goal_xy[2p+1].
 * The table of problem p.  Exactly one of two inputs gives the action a(s) of every state:
 *   policy  uint8[problems, S], 4-byte aligned: a(s) itself
 *   q       float[problems, S, 4], 16-byte aligned: a(s) is the first maximum by a strict '>' from action 0 on, the rule of
 *           lmaze_solve and lmaze_env_rollout_qlearn; a NaN never wins, a NaN in word 0 keeps action 0.  This is
 *           lmaze_q_first_max, the learner's rule, for a row that holds a NaN too; the host wrapper rollout_policy(q=) reads
 *           such a row as "no move" (greedy_table() gives it id 4) and agrees on every other row, so policy =
 *           greedy_table(q) scores exactly the walk rollout_policy(q=) takes
 * Both may be NULL when only distances are asked for.
 * Outputs, each nullable and 4-byte aligned, at least one required; all integers, so the result depends on no schedule:
 *   optimal  int32[problems, S]  the fewest steps after which an env started on s can have done set by the model: 1 if s owns
 *            a usable (not excluded) terminal pair, else 1 + the minimum over s's usable, non-terminal pairs of optimal[next];
 *            -1 where no terminal pair can be reached, and on walls
 *   steps    int32[problems, S]  the walk that takes a(s) in every state: the number of steps at which done is first set, -1 if
 *            that never happens -- the walk enters a cycle (a wall bump is a cycle of one), takes an excluded pair, meets a
 *            policy byte above 3, or starts on a wall.  This is the walk lmaze_rollout_policy takes at epsilon 0, with one
 *            exception: the step reads a byte above 3 as a move of (0, 0), and on the one cell where such a step pays the goal
 *            -- v0's 'X', on which only a loaded state stands, and v3's goal cell, which a walk can cross without being paid --
 *            the rollout sets done where steps says -1.  The (cell, no move) pair is not one of the model's four
 *   summary  int32[problems, 4]  reachable = #{s : optimal >= 1}, arrived = #{s : steps >= 1}, shortest = #{s : steps ==
 *            optimal >= 1}, excess = the sum over arrived s of (steps - optimal); without a table the last three are 0
 * An arriving walk visits distinct non-wall states, so steps <= (G - 2)^2 < S.
 * One launch of score_kernel, shaped as solve_kernel: a problem lives in LDS from its layout bytes to its results; a wave per
 * problem while G*G <= 256, four problems per workgroup and no workgroup barrier; a workgroup per problem above.  Distances:
 * Jacobi min-plus sweeps between two buffers, ended by the sweep that changes nothing, at most S of them.  Walk lengths:
 * pointer doubling between the same two buffers, ceil(log2 S) <= 12 rounds at most.  params->launch_hint, step_limit are not
 * read.
 * Refused, in this order: LMAZE_E_NULL params or layouts; LMAZE_E_GRID; LMAZE_E_VARIANT neither v0 nor v3; LMAZE_E_LAYOUT;
 * LMAZE_E_NULL goal_xy for v3; LMAZE_E_NULL all of optimal, steps and summary; LMAZE_E_NULL both policy and q given;
 * LMAZE_E_NULL steps without a table; LMAZE_E_COUNT problems outside [0, LMAZE_MAX_ENVS]; LMAZE_E_ALIGN q off 16 bytes,
 * goal_xy (v3) off 8, policy or an output off 4.  problems == 0 then returns 0 with nothing read.  A grid beyond 2^24 - 1
 * workgroups: hipErrorInvalidConfiguration.
 */
int lmaze_score(const LmazeParams* params, const uint8_t* layouts, const int32_t* goal_xy, int64_t problems, const uint8_t* policy,
                const float* q, int32_t* optimal, int32_t* steps, int32_t* summary, void* stream);

/*
 * The launch lmaze_score would queue, one line in text_host (HOST, len bytes), written by the code that launches, e.g.
 * "score_kernel<v0, wave, 4> grid=65 block=256 lds=8384 problems_per_workgroup=4" or "score_kernel<v3, workgroup, 2> ..."
 * (the third argument: cells per lane; the plan is lmaze_solve's).  Nothing is queued or dereferenced.  LMAZE_E_NULL params or
 * text_host NULL or len < 1, then lmaze_score's refusals of the params and of `problems`; an empty line for problems == 0.
 */
int lmaze_describe_score(const LmazeParams* params, int64_t problems, char* text_host, int32_t len);

/*
 * EXACT POLICY EVALUATION on the grid mazes: V^pi and Q^pi of the stochastic table a closed-loop rollout runs, in ONE launch;
 * no reference counterpart.  The linear twin of lmaze_solve: where that takes the maximum over the actions, this takes the
 * policy's expectation.  It gives the critic lmaze_advantages_table wants for a policy that explores, the expected return of a
 * half-learnt lmaze_env_rollout_qlearn table under the epsilon it is run with, and the Q^pi whose first maximum is the next
 * policy of policy iteration.
 * Problems, the model, the layout modes and the goals are lmaze_score's, word for word: problem p has S = G*G states,
 * s = x * G + y; the transition of lmaze_step_v0 / _v3 asked once per (cell, action) with a step count that trips no limit
 * (infinite horizon: the step limit is not in the model); the same wall, move and goal pairs; a pair is terminal exactly when
 * its reward equals reward_goal as float32; v0's sticky pairs are excluded; wall states and targets off the grid as in
 * lmaze_solve.  LMAZE_LAYOUT_SHARED: every problem reads the one layout and its own table (a population of tables on one maze,
 * v3 with one goal per problem, the goal-keyed tables); LMAZE_LAYOUT_PER_ENV: problem p reads layouts + p*G*G.  v3 reads
 * goal_xy[2p], goal_xy[2p+1].
 * The policy of problem p.  Exactly one of three inputs is given; each reduces to four integer weights w_0..w_3 per state, in
 * units of 2^-34:
 *   policy      uint8[problems, S] with epsilon_u32: lmaze_rollout_policy's rule (explore when r.x < epsilon_u32, then take
 *               action r.y >> 30): w_a = e + (a == policy[s] ? 4 * (2^32 - e) : 0), e = epsilon_u32.  A byte above 3 gives its
 *               greedy share to no action
 *   q           float[problems, S, 4], 16-byte aligned, with epsilon_u32: the same, the greedy action being the first maximum
 *               by a strict '>' from action 0 on -- lmaze_score's rule: a NaN never wins, a NaN in word 0 keeps action 0.
 *               That is lmaze_q_first_max, the learner's rule (lmaze_env_rollout_qlearn), for a row that holds a NaN too.
 *               The host wrapper rollout_policy(q=) reduces q by greedy_table() instead, which agrees on every row without a
 *               NaN and reads a row with one as id 4, "no move": to evaluate exactly the table rollout_policy(q=) runs, pass
 *               policy = greedy_table(q) (its id 4 then gives its greedy share to no action, as any byte above 3)
 *   thresholds  uint32[problems, S, 4], 16-byte aligned: lmaze_rollout_sample's rule, w_a = 4 * (s_a - s_(a-1)) with
 *               s_0 <= s_1 <= s_2 the words c_0, c_1, c_2 of the row in ascending order, s_(-1) = 0 and s_3 = 2^32; word 3 is
 *               ignored, epsilon_u32 is not read.  The sampler's action (r >= c0) + (r >= c1) + (r >= c2) counts the words r
 *               reaches and so does not depend on their order: w_a / 4 is the number of the 2^32 values of r that give
 *               action a, on a non-monotone row, which the sampler does not refuse either, as on a monotone one.  Every row
 *               sums to 2^34.  A row of probability 1 is stored as 1 - 2^-32 (see lmaze_rollout_sample): its action gets
 *               4 * (2^32 - 1) and action 3 gets 4
 * Probabilities, computed once per state before the first sweep:
 *   w'_a = w_a if the pair (s, a) is usable, 0 if the model excludes it (v0's sticky pairs);  W = w'_0 + w'_1 + w'_2 + w'_3,
 *   an integer;  p_a = fl(fl(w'_a) / fl(W)): both integers rounded to float32 (ties to even), one correctly rounded division.
 *   Where nothing is excluded, W = 2^34 and the division is an exact scaling.  W == 0 -- every pair
 *   that carries weight is excluded, or a byte above 3 at epsilon_u32 == 0 -- gives p_a = 0 for every action and v = 0.
 * So where lmaze_solve excludes a sticky pair from the maximum, the mass a policy puts on excluded pairs is RENORMALISED over the
 * usable ones: the step repeats the previous reward there and leaves the ball in place, which has no value of its own; the
 * evaluated policy is the one conditioned on taking a usable pair.
 * The sweep is Jacobi, in float32, every operation rounded on its own (round to nearest even, never a fused multiply-add):
 *   V_0 = v_init (problem p: v_init + p*S) or 0 when v_init is NULL
 *   Q_k(s, a) = lmaze_solve's: r(s, a) for a terminal pair, else r(s, a) + gamma * V_(k-1)(next); -INFINITY for an excluded pair
 *   V_k(s) = the sum over a = 0, 1, 2, 3, in that order, of p_a * Q_k(s, a), over the actions with w'_a != 0 only (so
 *            -INFINITY * 0 never occurs), starting from the first such term itself, not from 0 + term; 0 if there is none
 *   a state on a 'W' cell has q = 0 for all four actions and v = 0
 * A problem stops at the first sweep that leaves the bit pattern of every V(s) unchanged -- that sweep counts --, or, when
 * tol > 0, at the first sweep whose delta (below) is <= tol, compared as bit patterns so that a NaN delta never passes, or
 * after `sweeps` sweeps.  tol is not validated: a negative or NaN tol never stops a solve.  With epsilon_u32 == 0, policy =
 * lmaze_solve's policy and v_init = lmaze_solve's settled v, the first sweep changes no bit: V^pi is V* bit for bit.
 * Outputs, each nullable, one of q_out / v_out required:
 *   q_out       float[problems, S, 4]  Q_k of the last executed sweep; 16-byte aligned
 *   v_out       float[problems, S]     V_k
 *   sweeps_run  int32[problems]        sweeps executed
 *   delta       float[problems]        max_s |V_k(s) - V_(k-1)(s)| of the last executed sweep, as lmaze_solve's
 * One launch of evaluate_kernel, shaped as solve_kernel and with its plan: a problem lives in LDS for the whole solve (two V
 * buffers; the model and the four probabilities of a cell in registers, read from global memory once); a wave per problem while
 * G*G <= 256, four problems per workgroup and no workgroup barrier; a workgroup per problem above, one barrier per sweep.
 * params->launch_hint, step_limit are not read.
 * Refused, in this order: LMAZE_E_NULL params or layouts; LMAZE_E_GRID; LMAZE_E_VARIANT neither v0 nor v3; LMAZE_E_LAYOUT;
 * LMAZE_E_NULL goal_xy for v3; LMAZE_E_NULL both q_out and v_out NULL; LMAZE_E_NULL unless exactly one of policy, q and
 * thresholds is given; LMAZE_E_COUNT problems outside [0, LMAZE_MAX_ENVS] or sweeps < 1; LMAZE_E_ALIGN thresholds, q or q_out
 * off 16 bytes, goal_xy (v3) off 8, a float or int32 pointer off 4.  problems == 0 then returns 0 with nothing read.  gamma is
 * not validated.  A grid beyond 2^24 - 1 workgroups: hipErrorInvalidConfiguration.
 */
int lmaze_evaluate(const LmazeParams* params, const uint8_t* layouts, const int32_t* goal_xy, int64_t problems, const uint8_t* policy,
                   const float* q, uint32_t epsilon_u32, const uint32_t* thresholds, float gamma, int32_t sweeps, float tol,
                   const float* v_init, float* q_out, float* v_out, int32_t* sweeps_run, float* delta, void* stream);

/*
 * The launch lmaze_evaluate would queue, one line in text_host (HOST, len bytes), written by the code that launches, e.g.
 * "evaluate_kernel<v0, wave, 4> grid=65 block=256 lds=8208 problems_per_workgroup=4" or "evaluate_kernel<v3, workgroup, 2> ..."
 * (the third argument: cells per lane; the plan is lmaze_solve's).  Nothing is queued or dereferenced.  LMAZE_E_NULL params or
 * text_host NULL or len < 1, then lmaze_evaluate's refusals of the params and of `problems`; an empty line for problems == 0.
 */
int lmaze_describe_evaluate(const LmazeParams* params, int64_t problems, char* text_host, int32_t len);

/*
 * EXACT DISCOUNTED OCCUPANCY on the grid mazes: where the stochastic table lmaze_evaluate values spends its discounted time,
 * given where episodes start, in ONE launch; no reference counterpart.  lmaze_evaluate's adjoint: that propagates values
 * backward, V = r + gamma P V; this propagates mass forward, d = start + gamma P^T d.  With it the expected return of a table
 * is one dot product, <start, V> = <d_sa, r>, and the exact policy gradient of a softmax table is d(s) p_a(s) (Q(s,a) - V(s)).
 * The problems, the model, the layout modes, the goals, the rewards and the three policy inputs are lmaze_evaluate's,
 * unchanged: exactly one of policy or q (with epsilon_u32) or thresholds is given, and the probabilities are
 * p_a = fl(fl(w'_a) / fl(W)) with the weight on excluded pairs renormalised over the usable ones, computed once per state.
 * In the model a usable pair (s, a) that is not terminal leads to next(s, a): s + step(a) when the ball moves (the step leaves
 * it on another cell), else s; step(a) = -G, +G, -1, +1 for a = 0, 1, 2, 3.  A terminal pair absorbs its mass; an excluded
 * pair carries none.
 * For a cell c that is not 'W', computed once before the first sweep:
 *   win[a]  = p_a(c - step(a)) if that cell is on the grid -- judged by coordinates: for a = 2, 3 it lies in c's row -- and the
 *             pair (c - step(a), a) is usable, not terminal and moves the ball; else 0.  Each (c, a) has at most one source.
 *   wself   = the sum over a = 0, 1, 2, 3, in that order and from the first term itself, of p_a(c) over the pairs (c, a) that
 *             are usable, not terminal and leave the ball in place (wall bumps and clamped targets); 0 if there is none
 * The sweep is Jacobi, in float32, every product and sum rounded on its own (round to nearest even, never a fused multiply-add):
 *   D_0 = d_init (problem p: d_init + p*S) or 0 when d_init is NULL
 *   acc = 0
 *   for a = 0, 1, 2, 3:  if win[a] != 0:  acc = fl(acc + fl(win[a] * D_(k-1)(c - step(a))))
 *   if wself != 0:       acc = fl(acc + fl(wself * D_(k-1)(c)))
 *   D_k(c) = fl(start(c) + fl(gamma * acc));  on a 'W' cell D_k = 0 and its start is not read
 * The stops, sweeps_run and delta are lmaze_evaluate's: a problem stops at the first sweep that leaves the bit pattern of every
 * D(s) unchanged -- that sweep counts --, or, when tol > 0, at the first sweep whose delta is <= tol, compared as bit patterns,
 * or after `sweeps` sweeps.  From d_init = NULL and a start without a negative entry the sequence D_k is monotone
 * non-decreasing in every cell, because every rounded operation above is monotone on non-negative inputs (gamma >= 0); float32 has finitely
 * many values, so such a sequence becomes stationary and the exact stop is always reached.
 *   start       float[problems, S], required: the mass every sweep adds.  Not validated: it need not sum to 1
 * Outputs, each nullable, one of d_out / dsa_out required:
 *   d_out       float[problems, S]     D_k of the last executed sweep
 *   dsa_out     float[problems, S, 4]  fl(D_k(s) * p_a(s)); 16-byte aligned
 *   sweeps_run  int32[problems]        sweeps executed
 *   delta       float[problems]        max_s |D_k(s) - D_(k-1)(s)| of the last executed sweep, as lmaze_solve's
 * One launch of occupancy_kernel, shaped as evaluate_kernel and with lmaze_solve's plan: two D buffers in LDS; the model, the
 * four incoming weights, wself and start of a cell in registers.  The probabilities of the neighbours are exchanged once,
 * through the second buffer, before the first sweep.  params->launch_hint, step_limit are not read.
 * Refused, in this order: LMAZE_E_NULL params or layouts; LMAZE_E_GRID; LMAZE_E_VARIANT neither v0 nor v3; LMAZE_E_LAYOUT;
 * LMAZE_E_NULL goal_xy for v3; LMAZE_E_NULL both d_out and dsa_out NULL; LMAZE_E_NULL unless exactly one of policy, q and
 * thresholds is given; LMAZE_E_NULL start; LMAZE_E_COUNT problems outside [0, LMAZE_MAX_ENVS] or sweeps < 1; LMAZE_E_ALIGN
 * thresholds, q or dsa_out off 16 bytes, goal_xy (v3) off 8, a float or int32 pointer off 4.  problems == 0 then returns 0 with
 * nothing read.  gamma is not validated.  A grid beyond 2^24 - 1 workgroups: hipErrorInvalidConfiguration.
 */
int lmaze_occupancy(const LmazeParams* params, const uint8_t* layouts, const int32_t* goal_xy, int64_t problems, const uint8_t* policy,
                    const float* q, uint32_t epsilon_u32, const uint32_t* thresholds, const float* start, float gamma, int32_t sweeps,
                    float tol, const float* d_init, float* d_out, float* dsa_out, int32_t* sweeps_run, float* delta, void* stream);

/*
 * The launch lmaze_occupancy would queue, one line in text_host (HOST, len bytes), written by the code that launches, e.g.
 * "occupancy_kernel<v0, wave, 4> grid=65 block=256 lds=8208 problems_per_workgroup=4" (the third argument: cells per lane; the
 * plan is lmaze_solve's).  Nothing is queued or dereferenced.  LMAZE_E_NULL params or text_host NULL or len < 1, then
 * lmaze_occupancy's refusals of the params and of `problems`; an empty line for problems == 0.
 */
int lmaze_describe_occupancy(const LmazeParams* params, int64_t problems, char* text_host, int32_t len);

/*
 * MAZE GENERATION: `mazes` spanning-tree mazes of G x G cells, every one different, every free cell connected to its goal,
 * in ONE launch; no reference counterpart (the reference only has literal layouts).  The result is what LAYOUT_PER_ENV
 * entries and lmaze_solve read: layouts uint8[mazes, G, G] of the reference's cell characters.  Maze p of the call is the
 * global maze m = maze_base + p: a shard that passes its env offset as maze_base writes exactly its slice of the one-batch
 * result.  The maze is a function of (G, seed, m, loops_u32) alone, specified so that a numpy loop reproduces every byte:
 *   rooms   R = (G - 1) / 2 per side (integer division; G in [5, LMAZE_MAX_GRID], so R >= 2 and R*R <= 961).  Room (i, j),
 *           0 <= i, j < R, is cell (1 + 2i, 1 + 2j), its index r = i*R + j.  For even G row and column G - 2 hold no room
 *           and stay 'W'.
 *   edges   edge k = 2r joins room (i, j) to (i+1, j), exists iff i + 1 < R, its wall cell is (2 + 2i, 1 + 2j);
 *           edge k = 2r + 1 joins (i, j) to (i, j+1), exists iff j + 1 < R, its wall cell is (1 + 2i, 2 + 2j).
 *           k < 2 R*R <= 1922 < 2048.
 *   draws   one Philox4x32-10 call per room: counter (m_lo, m_hi, r, 0x40000000), key (seed_lo, seed_hi).  .x is the weight
 *           of edge 2r and .y of edge 2r + 1; .z is the loop draw of edge 2r and .w of edge 2r + 1.  The goal draw is the .x
 *           word of the call with r = R*R.  The last counter word cannot meet the reset or the exploration stream: those
 *           carry epoch_hi and epoch_hi ^ 0x80000000 there, with epochs far below 2^62.
 *   keys    key(k) = (weight(k) & 0xFFFFF800) | k: distinct within a maze.
 *   tree    the opened edges are the minimum spanning tree of the room graph under these keys.  Distinct keys make the tree
 *           unique, so the result does not depend on how it is computed; Kruskal in ascending key order is the definition.
 *   loops   if loops_u32 != 0, an existing non-tree edge is opened as well iff its loop draw < loops_u32 (unsigned);
 *           loops_u32 == 0 gives a perfect maze, R*R - 1 opened wall cells.
 *   goal    gr = (uint64(goal draw) * R*R) >> 32; room gr's cell becomes 'X'.
 *   bytes   room cells and the wall cells of opened edges are 'B', one of the rooms is 'X' instead, everything else -- the
 *           full border included -- is 'W'.  There is no 'S': v0's sticky pairs stay out of generated mazes.
 * By construction the layout has a full 'W' border and one 'X', and every free cell reaches the goal.
 *   layouts  uint8[mazes, G, G], 16-byte aligned; only written, and nothing outside [layouts, layouts + mazes*G*G)
 *   goal_xy  int32[mazes, 2], 8-byte aligned, nullable: the 'X' cell (x = row, y = column) of each maze, what lmaze_solve
 *            takes as a v3 goal
 * One launch of generate_kernel: a maze lives in LDS from its draws to its bytes, the tree found by Boruvka rounds (LDS
 * atomic minimum per component, hook, pointer jumping, relabel) whose loops run at most ceil(log2(R*R)) times each; a wave per
 * maze while G <= 33, four mazes per workgroup and no workgroup barrier; a workgroup per maze above.
 * Refused before anything is queued, in this order: LMAZE_E_NULL layouts; LMAZE_E_GRID grid outside [5, LMAZE_MAX_GRID];
 * LMAZE_E_COUNT mazes outside [0, LMAZE_MAX_ENVS], maze_base < 0, or maze_base + mazes beyond int64; LMAZE_E_ALIGN layouts off
 * 16 bytes or goal_xy off 8.  mazes == 0 then returns 0 with nothing written.  A grid beyond 2^24 - 1 workgroups:
 * hipErrorInvalidConfiguration.
 */
int lmaze_generate(int32_t grid, int64_t mazes, uint64_t seed, int64_t maze_base, uint32_t loops_u32, uint8_t* layouts,
                   int32_t* goal_xy, void* stream);

/*
 * The launch lmaze_generate would queue, one line in text_host (HOST, len bytes), written by the code that launches, e.g.
 * "generate_kernel<wave, 4> grid=4096 block=256 lds=26944 mazes_per_workgroup=4" or "generate_kernel<workgroup, 2> ..." (the
 * second argument: rooms per lane).  Nothing is queued or dereferenced.  LMAZE_E_NULL text_host NULL or len < 1, then
 * lmaze_generate's refusals of the grid and of `mazes`; an empty line for mazes == 0.
 */
int lmaze_describe_generate(int32_t grid, int64_t mazes, char* text_host, int32_t len);

/*
 * Reference-layout observation: replaces the 5-deep upsample loop (v0:217-234,
 * v3:295-301).  out[i, c, x*E+xx, y*E+yy] = float((obs[i,x,y] & channel_mask[c]) != 0).
 *   obs           int32[N,G,G]        compact planes
 *   channel_mask  int32[channels]     HOST array, one LMAZE_OBS_* bit per output plane,
 *                                     e.g. v0 {1,2,4,8}, v3 {8,1,4}
 *   out           float[N,channels,G*E,G*E], 16-byte aligned
 */
int lmaze_render_expanded(const int32_t* obs, int32_t grid, int32_t expansion,
                          const int32_t* channel_mask_host, int32_t channels, float* out,
                          int64_t n, void* stream);

/*
 * Episode statistics of a batch, off the step path (the reference only keeps goalCount, v0:24,195):
 * out4 int64[4] (device; zeroed by this call) =
 *   { #envs with done set, #envs with reward == reward_goal, sum of step_count over the done envs,
 *     sum of goal_count (0 when goal_count is NULL) }.
 * Integer sums, so the result does not depend on the order of the reduction.  A multi-GPU run sums
 * the four numbers over ranks with one all_reduce (the only collective this library ever needs).
 */
int lmaze_episode_stats(const uint8_t* done, const float* reward, const int32_t* step_count,
                        const int32_t* goal_count, float reward_goal, int64_t n, int64_t* out4, void* stream);

/*
 * Measured ceiling of the device this library runs on (SURVEY 8(d) asks for a measured fill / copy
 * ceiling beside the 8 TB/s figure): src == NULL fills `bytes` of dst with one 16-byte store per
 * thread in launch order; otherwise copies src -> dst the same way.  bytes % 16 == 0, both pointers
 * 16-byte aligned.  bench.py times it with events on the launch stream and reports
 * roofline.measured_ceiling; nothing on the step path calls it.  No reference counterpart.
 */
int lmaze_bandwidth_probe(const void* src, void* dst, int64_t bytes, void* stream);

/* ====================================================================================== */
/* Foveal variants: the agent sees a 5x5 window (a8 crop, a9 frame history of SURVEY 8a).  */
/*   v1 = gym_lmaze/envs/lmaze_env_v1.py   v2 = lmaze_env_v2.py   v4 = lmaze_env_v4.py       */
/* The observation is float[N,C,5,5]: exactly the reference's `retState` before its xE loop   */
/* (v1 C=4: v1:242-256; v2 C=5: v2:185-193; v4 C=7: v4:231-239); lmaze_expand_planes makes    */
/* the (C,35,35) reference layout from it.                                                    */
/* ====================================================================================== */
enum {
    LMAZE_VARIANT_V1 = 1, /* LmazeEnv_v1 (v1:114-200): 4-neighbour move, two reward streams, foveal goal */
    LMAZE_VARIANT_V2 = 2, /* LmazeEnv_v2 (v2:127-225): 25-way teleport inside the fovea, 5 layouts       */
    LMAZE_VARIANT_V4 = 4, /* LmazeEnv_v4 (v4:167-272): v2 + float visit-map plane                        */
    LMAZE_VARIANT_V5 = 5, /* LmazeEnv_v5 (v5:187-292): two-level planner / local loop, 8-tuple return    */
    LMAZE_VARIANT_V6 = 6  /* LmazeEnv_v6: v5 + safeFovealGoal (v6:505-523); same step rules             */
};

#define LMAZE_FOVEA 5
#define LMAZE_MAX_LAYOUTS 16

typedef struct LmazeFovealParams {
    int32_t variant;            /* LMAZE_VARIANT_V1 / V2 / V4                                          */
    int32_t grid;               /* G (v1: 14, v1:22; v2/v4: 18)                                        */
    int32_t n_layouts;          /* rows of the layout table uint8[L,G,G] (v1: 1; v2/v4: 5, v2:309-405) */
    int32_t step_limit;         /* v1: done at stepCount == 200 (v1:295); v2/v4: > 50 (v2:222);
                                   v5/v6: localDone at stepCount >= 10 (v5:45,267)                     */
    int32_t foveal_step_limit;  /* v1: fovealStepCount == 10 (v1:309); v5/v6: >= 50 ends the episode
                                   (v5:46,269-271); unused by v2/v4                                    */
    float reward_wall;          /* negativeNominal -1.0                                                 */
    float reward_move;          /* positiveNominal v1 +0.01 (v1:28); v2/v4 -0.01 (v2:47)               */
    float reward_goal;          /* positiveFull    v1 1.0 (v1:29);   v2/v4 100.0                       */
    int32_t launch_hint;        /* 0 = library default launch policy; else bits 0-3 = workgroups per CU
                                   (1..8, 0 = no cap), bits 4-7 = envs per workgroup, 2: 32, 3: 64, 4: 128,
                                   5: 256 (anything else = default), bits 8-9 = chunks of that many envs a
                                   workgroup takes, minus one.  Performance only, never results
                                   (lmaze_foveal_launch.h foveal_plan); other bits 0.                    */
} LmazeFovealParams;

/* Device pointers, one element per env; entries a variant does not use may be NULL. */
typedef struct LmazeFovealBuffers {
    int32_t* ball_xy;           /* [N,2] ball_x0, ball_y0 (window centre)                               */
    int32_t* goal_xy;           /* [N,2] goal_x, goal_y             v2, v4 (v1 reads 'X' off the layout) */
    int32_t* fgoal_xy;          /* [N,2] f_goal_x, f_goal_y         v1 (v1:104-110)                     */
    int32_t* layout_id;         /* [N]   row of the layout table    v2, v4 (v2:306)                     */
    int32_t* step_count;        /* [N]   stepCount                                                      */
    int32_t* foveal_step_count; /* [N]   fovealStepCount            v1 (not reset by reset(), v1:94)    */
    float* reward;              /* [N]   originalReward                                                 */
    float* foveal_reward;       /* [N]   fovealReward               v1                                  */
    uint8_t* done;              /* [N]                                                                  */
    uint8_t* foveal_done;       /* [N]   isFovealEpisodeFinished()  v1 (v1:308-324)                     */
    float* visit;               /* visit map state[2] of v4, v5, v6 (v4:116-119, v5:313-318) in the library's own
                                   CLOCK-RELATIVE, TILED form: lmaze_foveal_visit_bytes(G, N) bytes, 64-byte
                                   aligned, opaque to the caller -- see "The visit map" below; the reference's
                                   float[N,G,G] comes out of lmaze_foveal_materialise_visit                     */
    float* obs;                 /* [N,C,5,5], 16-byte aligned (v5/v6: the foveal observation, C = 7)    */
    /* v5 / v6 only (v5:62-78).  For them: reward = globalReward, foveal_reward = originalReward (the
     * local stream), done = globalDone, foveal_done = localDone, fgoal_xy = f_goal_x0/y0.               */
    int32_t* ball1_xy;          /* [N,2] ball_x1, ball_y1 (previous ball, v5:193-194)                   */
    int32_t* fovea_xy;          /* [N,4] fovea_x0, fovea_y0, fovea_x1, fovea_y1                         */
    int32_t* last_xy;           /* [N,2] window centre `retStatelast` is a view of (v5:322-323,344-346) */
    int32_t* foveal_goal;       /* [N]   index 0..24 of the one-hot fovealGoal plane (v5:166-169)        */
    float* obs_local;           /* [N,4,5,5] buildLocalObservation (v5:356-380), 16-byte aligned        */
    int32_t* visit_clock;       /* [N]   v4, v5, v6: bits 0-7 the whole-plane halvings the map has taken in its current
                                   frame; the library keeps a tag in the upper bits (v5/v6: which window centre the
                                   env's "previous window" record behind the tiles belongs to).  Opaque, as `visit`. */
} LmazeFovealBuffers;

/*
 * The visit map (v4:116-119,211-214; v5:313-318).  The reference keeps float32[G,G] per env and, on every update,
 * halves the WHOLE plane after adding 1 to the 5x5 window: state[2] = (state[2] + window) / 2.  Only window cells
 * are ever observable, so this library stores each cell relative to a per-env clock instead:
 *     stored s = v * 2^(clock - 126)      v = the reference's float32 value, clock = visit_clock[i]
 * "halve the whole plane" is clock += 1 and touches no cell; a window cell takes v' = fl32((v + 1) / 2) -- one
 * float32 add and an exact halving, which is the reference's float64 round trip rounded once -- and is stored
 * under the new clock.  Reading a cell back is an exponent subtraction while v stays in the normal range; below
 * 2^-126 the reference's own sequence of round-to-nearest-even halvings is replayed on the bit pattern (at most 25
 * steps to 0), so cells that were last seen hundreds of steps ago still come out bit-identical.  When a clock
 * reaches 250 the env's map is rewritten once in true values (clock := 126); reset() writes zeros (clock := 0).
 * Layout: tiles of 4x4 cells (64 bytes, one memory sector), ceil(G/4)^2 tiles per env, row-major tiles, row-major
 * cells inside a tile; a 5x5 window is always exactly 2x2 tiles (3 memory lines of 128 bytes on average).  A step
 * reads ten and writes back at most ten 16-byte tile rows of an env's map instead of streaming all 4*G*G bytes
 * twice.  Behind the tiles of the whole batch sit N records of 28 words: the true values of the window the
 * observation shows as "previous" (v5/v6 show it unchanged for up to ten steps: 112 contiguous bytes instead of a
 * second gather).  lmaze_foveal_visit_bytes() covers both.
 */
int64_t lmaze_foveal_visit_bytes(int32_t grid, int64_t n);

/* As lmaze_describe_step, for lmaze_foveal_step (auto_reset != 0: lmaze_foveal_step_autoreset; v5/v6:
 * lmaze_v5_hier_step). */
int lmaze_describe_foveal_step(const LmazeFovealParams* params, int64_t n, int32_t auto_reset, char* text_host, int32_t len);

/* out float[N,G,G] = the reference's state[2] of every env (true values, row-major), from the clock-relative
 * tiles.  Off the step path (tests, LmazeEnv_v4.state, checkpoints). */
int lmaze_foveal_materialise_visit(const LmazeFovealParams* params, const LmazeFovealBuffers* bufs, float* out,
                                   int64_t n, void* stream);

/* The inverse: take float[N,G,G] true values (e.g. the reference's own state[2]) into the tiled form;
 * visit_clock[i] := 126, the frame in which stored == true value. */
int lmaze_foveal_load_visit(const LmazeFovealParams* params, const LmazeFovealBuffers* bufs, const float* in,
                            int64_t n, void* stream);

/*
 * One step() of N foveal envs (v1:114-200 | v2:127-225 | v4:167-272).
 *   layouts  uint8[L,G,G] device; action int32[N] (v1: 0..3 else no move; v2/v4: 0..24 =
 *   5*row+col of the target cell inside the window; the reference raises IndexError outside
 *   that range before it changes anything, here such an id leaves the env -- state and obs --
 *   untouched).
 * Layouts need the reference's 2-cell (v1) / 4-cell (v2, v4) 'W' padding so the window never
 * leaves the array (v1:40-53, v2:309-326).
 */
int lmaze_foveal_step(const LmazeFovealParams* params, const uint8_t* layouts, const int32_t* action,
                      const LmazeFovealBuffers* bufs, int64_t n, void* stream);

/*
 * step() with the reset fused in front (v1, v2, v4): an env whose done[i] is set ON ENTRY is first reset
 * exactly as lmaze_foveal_reset(mask = done, place = 1, seed, epoch, env_base) would, then takes this step's
 * action -- bit-identical to the two calls, one launch.  (A masked reset launch per step costs +78 % on v2
 * and +39 % on v4 at 1M envs; fused it is free.)  v5/v6 episodes restart through plannerStep and are not
 * covered.  epoch_in_dev / epoch_out_dev: the device-resident epoch, as for lmaze_step_v0_autoreset.
 */
int lmaze_foveal_step_autoreset(const LmazeFovealParams* params, const uint8_t* layouts, const int32_t* action,
                                const LmazeFovealBuffers* bufs, int64_t n, uint64_t seed, uint64_t epoch,
                                int64_t env_base, const uint64_t* epoch_in_dev, uint64_t* epoch_out_dev,
                                void* stream);

/*
 * reset() of the envs with mask[i] != 0 (NULL = all): step_count = 0, rewards = -0.0, done
 * flags cleared, visit map zeroed and visit_clock = 0 (v4: then (0 + window)/2, v4:116-119), and the reset
 * observation written (v1: global view v1:204-238; v2/v4: [window, zero action plane, window],
 * v2:109-110).  place != 0 also draws the placement on the device with Philox4x32-10 keyed by
 * (seed, env_base + i, epoch): v1 ball = the 'S' cell (v1:82-84); v2 goal, ball on the CURRENT
 * layout and only then a new layout_id (the reset-order quirk of v2:90-92); v4 layout_id first
 * (v4:97-104).  place == 0 keeps the caller's ball/goal/layout_id (e.g. the reference's own
 * draws).  Unmasked envs are untouched, their obs included.
 */
int lmaze_foveal_reset(const LmazeFovealParams* params, const uint8_t* layouts, const uint8_t* mask,
                       int32_t place, uint64_t seed, uint64_t epoch, int64_t env_base,
                       const LmazeFovealBuffers* bufs, int64_t n, void* stream);

/*
 * v1 setFovealGoal(i, j) (v1:104-110) for the envs with mask[i] != 0 (NULL = all):
 * f_goal = ball + (i, j) - 2, fovealStepCount = 0, obs = local view (v1:242-279).
 *   ij int32[N,2]
 */
int lmaze_v1_set_foveal_goal(const LmazeFovealParams* params, const uint8_t* layouts, const int32_t* ij,
                             const uint8_t* mask, const LmazeFovealBuffers* bufs, int64_t n, void* stream);

/*
 * v5/v6 plannerStep(goal) (v5:158-182) for the envs with mask[i] != 0 (NULL = all):
 * stepCount = 0, globalReward = -0.0, localDone = False, foveal goal = ball + (goal/5, goal%5) - 2,
 * fovea history shifted once fovealStepCount > 0, fovealStepCount += 1, obs_local written.
 * goal int32[N] in 0..24; the reference raises IndexError half-way through for any other value,
 * here such an env is left untouched.  lmaze_foveal_step / lmaze_foveal_reset take these variants
 * too: step() = v5:187-292 with actions 0:(+1,0) 1:(-1,0) 2:(0,+1) 3:(0,-1) (v5:205-217; the
 * opposite sign convention to v0), writing obs (foveal, v5:306-348) and obs_local.  Where the
 * reference's buildLocalObservation indexes outside its 5x5 frame (ball more than 2 cells right /
 * below fovea_1) it raises IndexError AFTER the state was updated; the kernel leaves that one-hot
 * plane empty and the state is the reference's.
 */
int lmaze_v5_planner_step(const LmazeFovealParams* params, const uint8_t* layouts, const int32_t* goal,
                          const uint8_t* mask, const LmazeFovealBuffers* bufs, int64_t n, void* stream);

/*
 * The two-level loop of v5/v6 as ONE launch per env-step: what a caller of the reference does around step() --
 *     if globalDone: reset()                       (v5:104-150)
 *     if localDone or it was just reset: plannerStep(goal)   (v5:158-182)
 *     step(action)                                 (v5:187-292)
 * -- for every env, keyed on the done[i] / foveal_done[i] flags ON ENTRY.  Bit-identical to
 * lmaze_foveal_reset(mask = done, place = 1, seed, epoch, env_base), then lmaze_v5_planner_step(planner_goal,
 * mask = done | foveal_done), then lmaze_foveal_step(action): state, visit map, obs and obs_local.  planner_goal
 * int32[N] is read for every env and used by those that take the plannerStep (a value outside 0..24 skips that
 * env's plannerStep, as lmaze_v5_planner_step does).  epoch_in_dev / epoch_out_dev: the device-resident epoch, as
 * for lmaze_step_v0_autoreset.
 */
int lmaze_v5_hier_step(const LmazeFovealParams* params, const uint8_t* layouts, const int32_t* action,
                       const int32_t* planner_goal, const LmazeFovealBuffers* bufs, int64_t n, uint64_t seed,
                       uint64_t epoch, int64_t env_base, const uint64_t* epoch_in_dev, uint64_t* epoch_out_dev,
                       void* stream);

/*
 * T steps of N foveal envs over pre-generated int32[T,N] tensors (row t = step t) as ONE launch, exactly what T calls
 * would do (v1:114-200, v2:127-225, v4:167-272, v5:104-292):
 *   planner_goals == NULL, auto_reset == 0   T x lmaze_foveal_step(actions[t])
 *   planner_goals == NULL, auto_reset != 0   T x lmaze_foveal_step_autoreset(actions[t]), step t drawing with epoch + t
 *                                            (v1, v2, v4)
 *   v5/v6, planner_goals != NULL             T x lmaze_v5_hier_step(actions[t], planner_goals[t], epoch + t)
 * with bit-identical state, visit map, obs and obs_local at the end.  The caller advances its epoch by T whenever resets
 * are possible.  reward_t / done_t float[T,N] / uint8[T,N] and, v1 and v5/v6, foveal_reward_t / foveal_done_t (all
 * nullable) receive every step's reward / done / foveal_reward / foveal_done row -- what the buffers of `bufs` hold after
 * that step.  A workgroup sets up its layout tables once and runs all T steps of its chunk of envs before it takes the
 * next chunk; the per-env state, visit tiles and observations go through this CU's caches between steps.
 * The plain v5/v6 step (no planner goals) has no one-launch form: compiled so, it spills at 4 waves per SIMD, its step
 * kernel's floor; call lmaze_foveal_step T times.
 * T == 0 or n == 0: 0, nothing read.  LMAZE_E_COUNT: T < 0 or n outside [0, LMAZE_MAX_ENVS].  LMAZE_E_NULL: a required
 * pointer is NULL (planner_goals included for v5/v6 with auto_reset != 0).  LMAZE_E_VARIANT: planner_goals for v1/v2/v4,
 * or none for v5/v6.
 * launch_hint: bits 4-7 = 2 / 3 / 4: 32 / 64 / 128 envs per workgroup (other codes: the default), bits 8-9 chunks per
 * workgroup - 1, bits 0-3 workgroups per CU, as for the step; they never change results.
 */
int lmaze_foveal_rollout(const LmazeFovealParams* params, const uint8_t* layouts, const int32_t* actions,
                         const int32_t* planner_goals, int32_t T, const LmazeFovealBuffers* bufs, int64_t n,
                         int32_t auto_reset, uint64_t seed, uint64_t epoch, int64_t env_base,
                         float* reward_t, uint8_t* done_t, float* foveal_reward_t, uint8_t* foveal_done_t,
                         void* stream);

/*
 * lmaze_foveal_rollout that also RECORDS every k-th step's observations, in one launch.  Same arguments, then:
 *   obs_t        float[T / obs_every, N, C, 5, 5], 16-byte aligned: slot j = what bufs->obs holds after step
 *                (j + 1) * obs_every - 1 of the T step calls (fused resets included; an env whose step is skipped -- an
 *                out-of-range v2/v4 action -- keeps, and records, its previous observation)
 *   obs_local_t  float[T / obs_every, N, 4, 5, 5], 16-byte aligned, nullable: the same for bufs->obs_local (v5/v6 with
 *                planner goals; LMAZE_E_VARIANT for the other variants)
 *   obs_every    k >= 1 (there is no final-planes-only form here)
 * The running obs / obs_local are still written every step; final state, visit map, obs, obs_local and the rows are
 * bit-identical to lmaze_foveal_rollout, whose refusals (the plain v5/v6 step included) apply unchanged.  Refused first,
 * before anything is queued: LMAZE_E_COUNT obs_every < 1; LMAZE_E_NULL obs_t NULL while T / obs_every > 0;
 * LMAZE_E_ALIGN obs_t or obs_local_t not 16-byte aligned.  LMAZE_E_GRID: v5/v6 at G != 18, v1 at G != 14 (those
 * recording forms would spill at the rollouts' 4 / 6 waves per SIMD; record through T step calls instead).
 */
int lmaze_foveal_rollout_obs(const LmazeFovealParams* params, const uint8_t* layouts, const int32_t* actions,
                             const int32_t* planner_goals, int32_t T, const LmazeFovealBuffers* bufs, int64_t n,
                             int32_t auto_reset, uint64_t seed, uint64_t epoch, int64_t env_base,
                             float* reward_t, uint8_t* done_t, float* foveal_reward_t, uint8_t* foveal_done_t,
                             float* obs_t, float* obs_local_t, int32_t obs_every, void* stream);

/* As lmaze_describe_foveal_step, for lmaze_foveal_rollout (two_level != 0: v5/v6 with planner goals, the only v5/v6
 * form); the text also names T. */
int lmaze_describe_foveal_rollout(const LmazeFovealParams* params, int64_t n, int32_t T, int32_t auto_reset,
                                  int32_t two_level, char* text_host, int32_t len);

/* The same for lmaze_foveal_rollout_obs with this obs_every: the recording form of the kernel ("..., obs_t>" in the text).
 * Its refusals are the entry point's: LMAZE_E_COUNT obs_every < 1; LMAZE_E_GRID v5/v6 at G != 18, v1 at G != 14. */
int lmaze_describe_foveal_rollout_obs(const LmazeFovealParams* params, int64_t n, int32_t T, int32_t auto_reset,
                                      int32_t two_level, int32_t obs_every, char* text_host, int32_t len);

/*
 * CLOSED-LOOP foveal rollout (v1, v2, v4): lmaze_foveal_rollout / lmaze_foveal_rollout_obs with a tabular epsilon-greedy
 * policy inside the kernel instead of a pre-generated action tensor.  Replaces the user loop of T x (look the action up by
 * layout row and ball, mix in exploration, lmaze_foveal_step / lmaze_foveal_step_autoreset) -- three or more launches per
 * step -- by ONE launch; the action selection itself has no reference counterpart.  The arguments of lmaze_foveal_rollout
 * with `actions` / `planner_goals` replaced by
 *   policy       uint8[L*G*G] (L = 1 for v1): the greedy action id of every key, passed through unchanged, nothing is
 *                validated.  An id means what it means to lmaze_foveal_step -- v1: 0..3, anything else is no move; v2/v4:
 *                0..24, anything else leaves the env untouched (after a fused reset: reset, then no step)
 *   epsilon_u32  as in lmaze_rollout_policy; 0: nothing is drawn
 * and, beside reward_t / done_t (v1: foveal_reward_t / foveal_done_t too, as in lmaze_foveal_rollout),
 *   actions_t    int32[T,N], nullable: the action step t took
 *   key_t        int32[T,N], nullable: the key it was looked up with
 *   obs_t, obs_every   obs_every == 0: no recording, obs_t must be NULL (the running bufs->obs is still written every step;
 *                there is no final-observation-only form here either); obs_every = k >= 1: the slots float[T / k, N, C, 5, 5]
 *                exactly as in lmaze_foveal_rollout_obs
 * Env i (global index e = env_base + i) at step t, ep = epoch + t:
 *   1. auto_reset != 0 and the env done on entry: the fused reset of lmaze_foveal_step_autoreset, same draw, epoch ep (v2:
 *      placed on the current layout, then layout_id redrawn; v4: layout_id first);
 *   2. key = lid * G^2 + bx * G + by of the state after that reset: lid the layout row the step will use, clamped to
 *      0..L-1 (0 for v1), bx and by clamped to 0..G-1;
 *   3. action = policy[key]; if epsilon_u32 != 0, r = the exploration draw of lmaze_rollout_policy -- Philox4x32-10(counter
 *      (e_lo, e_hi, ep_lo, ep_hi ^ 0x80000000), key (seed_lo, seed_hi)) -- and where r.x < epsilon_u32 the action becomes
 *      (r.y * A) >> 32 with A = 4 for v1 and A = 25 for v2/v4 (A = 4: r.y >> 30, the grid envs' rule);
 *   4. the transition, visit-map update (v4) and observation of lmaze_foveal_step with that action;
 *   5. actions_t[t,i] = the action, key_t[t,i] = the key -- for every env, skipped ones included.
 * The caller advances its epoch by T whether or not auto_reset is set: exploration consumes epochs too.
 * The table is staged in LDS once per workgroup, behind the layout characters, when L*G*G <= 8192 bytes (196 B for v1,
 * 1 620 B for the five 18 x 18 layouts of v2/v4); above that it is read from global memory, one byte per env-step.  This is
 * a rule, not a measurement; lmaze_describe_foveal_rollout_policy reports it as table=lds / table=global.
 * v5/v6 are refused: their two-level step sits at 128 VGPRs and a closed loop there needs two tables (action and planner
 * goal) -- lmaze_v5_rollout_policy is that loop.  No grid size is refused: every form exists for any G (v1's recording form at G != 14 runs at 4 waves per SIMD).
 * Refused before anything is queued, in this order:
 *   1. the recording request: LMAZE_E_COUNT obs_every < 0, or obs_t given with obs_every == 0; LMAZE_E_NULL obs_t missing
 *      while T / obs_every > 0; LMAZE_E_ALIGN obs_t not 16-byte aligned;
 *   2. the params' own: LMAZE_E_NULL params; LMAZE_E_VARIANT an unknown variant; LMAZE_E_GRID; LMAZE_E_LAYOUT n_layouts or
 *      launch_hint;
 *   3. LMAZE_E_VARIANT v5/v6;
 *   4. LMAZE_E_COUNT T < 0 or n outside [0, LMAZE_MAX_ENVS];
 *   5. T == 0 or n == 0 returns 0 with nothing read;
 *   6. LMAZE_E_NULL a required pointer (layouts, bufs and its members as for lmaze_foveal_step, policy), then LMAZE_E_ALIGN
 *      as lmaze_foveal_step.
 * launch_hint bits 0-3, 4-7 and 8-9 as in lmaze_foveal_rollout; they never change results.
 */
int lmaze_foveal_rollout_policy(const LmazeFovealParams* params, const uint8_t* layouts, const uint8_t* policy,
                                uint32_t epsilon_u32, int32_t T, const LmazeFovealBuffers* bufs, int64_t n,
                                int32_t auto_reset, uint64_t seed, uint64_t epoch, int64_t env_base,
                                float* reward_t, uint8_t* done_t, float* foveal_reward_t, uint8_t* foveal_done_t,
                                int32_t* actions_t, int32_t* key_t, float* obs_t, int32_t obs_every, void* stream);

/* As lmaze_describe_foveal_rollout, for lmaze_foveal_rollout_policy with this obs_every (0: no recording):
 * "foveal_rollout_policy_kernel<v2, 32, 18, fused-reset, obs_t> table=lds T=24 grid=...".  LMAZE_E_NULL text_host NULL or
 * len < 1, then the entry point's refusals 1-4 in their order (obs_every > 0 stands for a given obs_t); an empty line for
 * T == 0 or n == 0.  Nothing is queued or dereferenced. */
int lmaze_describe_foveal_rollout_policy(const LmazeFovealParams* params, int64_t n, int32_t T, int32_t auto_reset,
                                         int32_t obs_every, char* text_host, int32_t len);

/*
 * SAMPLING closed-loop foveal rollout (v1, v2, v4): lmaze_foveal_rollout_policy with a categorical table policy instead of the
 * epsilon-greedy one -- every env-step draws its action from the distribution of its key, the form that produces REINFORCE,
 * actor-critic and Boltzmann data in one launch.  Replaces the user loop of T x (gather the key's row, compare a draw,
 * lmaze_foveal_step / lmaze_foveal_step_autoreset).  The arguments of lmaze_foveal_rollout_policy with `policy, epsilon_u32`
 * replaced by
 *   thresholds   const uint32_t*, 16-byte aligned, one row of cumulative thresholds per key:
 *                v1     uint32[G*G, 4], the grid format of lmaze_rollout_sample: words 0-2 are c0 <= c1 <= c2, word 3 is
 *                       reserved -- it is loaded with the rest and ignored;
 *                v2/v4  uint32[L*G*G, 24], 96 bytes per key, c0 <= ... <= c23, six 128-bit reads.
 * Env i (global index e = env_base + i) at step t, ep = epoch + t:
 *   1. the fused reset exactly as in lmaze_foveal_rollout_policy (same draw, same epoch);
 *   2. the key exactly as there: lid * G^2 + bx * G + by after the reset, each part clamped;
 *   3. r = the .x word of the closed loop's exploration draw -- Philox4x32-10(counter (e_lo, e_hi, ep_lo, ep_hi ^ 0x80000000),
 *      key (seed_lo, seed_hi)), the reset draw's counter with the top bit of its last word flipped -- and
 *      action = sum over k of (r >= c_k), unsigned compares, over the 3 (v1) or 24 (v2/v4) thresholds of the key's row.  The
 *      action is drawn on every env-step and is always in 0..A-1 (A = 4 or 25), so no env is ever skipped.  The table is not
 *      validated: a row that is not monotone still yields the action this formula gives (an implementation by binary
 *      search is not equivalent);
 *   4. the transition, visit-map update (v4) and observation of lmaze_foveal_step with that action;
 *   5. actions_t[t,i] and key_t[t,i] are written for every env; the reward and done rows (both streams for v1) and
 *      obs_t / obs_every are as in lmaze_foveal_rollout_policy.
 * Action k is taken with probability (c_k - c_(k-1)) / 2^32, c_(-1) = 0, c_(A-1) = 2^32.
 * The caller advances its epoch by T whether or not auto_reset is set.
 * The table is staged in LDS once per workgroup, behind the layout characters, when its size in bytes is at most 16 384
 * (lmaze_rollout_sample's figure): v1 at 14 x 14 (3 136 B) and a single v2/v4 layout up to 13 x 13 (16 224 B).  Above that --
 * the five 18 x 18 layouts of v2/v4 are 155 520 B -- it is read from global memory, the key's six reads requested together.
 * A rule, not a measurement; lmaze_describe_foveal_rollout_sample reports it as table=lds / table=global.
 * v5/v6 are refused with LMAZE_E_VARIANT.  No grid size is refused: every form exists for any G.
 * Refused before anything is queued: the refusals of lmaze_foveal_rollout_policy, in its order, with `thresholds` in the
 * place of `policy`; a table that is not 16-byte aligned is LMAZE_E_ALIGN, after the alignment refusals of
 * lmaze_foveal_step.  launch_hint bits 0-3, 4-7 and 8-9 as in lmaze_foveal_rollout; they never change results.
 */
int lmaze_foveal_rollout_sample(const LmazeFovealParams* params, const uint8_t* layouts, const uint32_t* thresholds, int32_t T,
                                const LmazeFovealBuffers* bufs, int64_t n, int32_t auto_reset, uint64_t seed, uint64_t epoch,
                                int64_t env_base, float* reward_t, uint8_t* done_t, float* foveal_reward_t, uint8_t* foveal_done_t,
                                int32_t* actions_t, int32_t* key_t, float* obs_t, int32_t obs_every, void* stream);

/* As lmaze_describe_foveal_rollout_policy, for lmaze_foveal_rollout_sample:
 * "foveal_rollout_sample_kernel<v2, 32, 18, fused-reset, obs_t> table=global T=24 grid=...".  The same refusals and empty
 * lines.  Nothing is queued or dereferenced. */
int lmaze_describe_foveal_rollout_sample(const LmazeFovealParams* params, int64_t n, int32_t T, int32_t auto_reset,
                                         int32_t obs_every, char* text_host, int32_t len);

/*
 * CLOSED-LOOP TWO-LEVEL rollout (v5, v6): lmaze_foveal_rollout / lmaze_foveal_rollout_obs over the two-level step
 * (lmaze_v5_hier_step, v5:104-292) with BOTH policies inside the kernel -- a tabular epsilon-greedy planner that picks the
 * foveal goal and a tabular epsilon-greedy controller that walks to it -- instead of pre-generated action and planner-goal
 * tensors.  Replaces the user loop of T x (two gathers, two epsilon mixes, lmaze_v5_hier_step) by ONE launch; the selections
 * themselves have no reference counterpart.  The arguments of lmaze_foveal_rollout_obs with `actions`, `planner_goals` and
 * `auto_reset` replaced by
 *   controller           uint8[100] (controller_key 0) or uint8[100 L G G] (controller_key 1): the greedy action id of every
 *                        controller key, passed through unchanged; 0..3 as lmaze_foveal_step reads them, anything above 3 is
 *                        no move
 *   controller_key       0 "offset": the key is the foveal goal's offset from the ball; 1 "cell": planner key * 100 + offset,
 *                        the controller's full Markov state.  A run-time argument, uniform over the launch
 *   epsilon_u32          the controller's exploration rate, as in lmaze_rollout_policy
 *   planner              uint8[L G G]: the greedy goal id of every planner key, passed through unchanged; 0..24 = 5 row + col
 *                        of the goal in the window, anything above 24 skips the plannerStep (lmaze_v5_planner_step)
 *   planner_epsilon_u32  the planner's exploration rate, likewise
 * and, beside reward_t / done_t / foveal_reward_t / foveal_done_t (all nullable),
 *   actions_t, key_t        int32[T,N], nullable: the action step t took and the controller key it was looked up with
 *   goals_t, goal_key_t     int32[T,N], nullable: the goal and the planner key of the envs that took a plannerStep at step t,
 *                           -1 in both where none was due -- table_stats skips those entries by construction
 *   obs_t, obs_local_t, obs_every   obs_every == 0: no recording, both must be NULL; obs_every = k >= 1: the slots exactly
 *                           as in lmaze_foveal_rollout_obs (obs_local_t nullable)
 * Env i (global index e = env_base + i) at step t, ep = epoch + t, gd / ld its done / foveal_done ON ENTRY:
 *   1. if epsilon_u32 | planner_epsilon_u32 is non-zero, r = the exploration draw of lmaze_rollout_policy, drawn once --
 *      Philox4x32-10(counter (e_lo, e_hi, ep_lo, ep_hi ^ 0x80000000), key (seed_lo, seed_hi)); nothing is drawn when both
 *      are 0;
 *   2. gd: the reset of lmaze_v5_hier_step, same draw, epoch ep (v5:104-150);
 *   3. gd | ld: the planner steps.  kp = lid * G^2 + bx * G + by of the state after that reset, lid clamped to 0..L-1, bx and
 *      by to 0..G-1; g = planner[kp]; if planner_epsilon_u32 != 0 and r.z < planner_epsilon_u32, g = (r.w * 25) >> 32; then
 *      plannerStep(g) as lmaze_v5_hier_step does it (v5:158-182) -- g > 24 skips it and the env goes on with its old goal.
 *      goals_t[t,i] = g, goal_key_t[t,i] = kp; where no plannerStep was due both are -1;
 *   4. the controller key, from the state after 3.: ox = clamp(fgoal_x - ball_x + 4, 0, 9), oy likewise, d = ox * 10 + oy (an
 *      undisturbed env has the offset in -4..5; the clamp only matters after a skipped plannerStep or for a loaded state);
 *      kc = d for controller_key 0 and kp' * 100 + d for controller_key 1, kp' the formula of 3. on the current state;
 *   5. a = controller[kc]; if epsilon_u32 != 0 and r.x < epsilon_u32, a = r.y >> 30; then step(a) as lmaze_v5_hier_step does it
 *      (v5:187-292), a > 3 is no move.  actions_t[t,i] = a, key_t[t,i] = kc, for every env;
 *   6. reward and done rows of both streams, visit map, obs, obs_local and the recorded slots as in lmaze_foveal_rollout_obs.
 * The caller advances its epoch by T.
 * Each table of at most 8192 bytes is staged in LDS once per workgroup, behind the layout characters (the controller's first,
 * then the planner's), its dwords requested beside the layout loads: the 100-byte offset table always, the planner table of
 * the five 18 x 18 layouts (1 620 B) too; a larger one -- a cell-mode controller of those layouts is 162 000 B, a planner table
 * of 16 layouts of 24 x 24 is 9 216 B -- is read from global memory, one byte per use.  This is a rule, not a measurement;
 * lmaze_describe_v5_rollout_policy reports it as controller=lds|global planner=lds|global.
 * No grid size is refused: the row and the recording form exist for any G, at 32, 64 and 128 envs per workgroup.
 * Refused before anything is queued, in the order of lmaze_foveal_rollout_policy:
 *   1. the recording request: LMAZE_E_COUNT obs_every < 0, or obs_t / obs_local_t given with obs_every == 0; LMAZE_E_NULL obs_t
 *      missing while T / obs_every > 0; LMAZE_E_ALIGN obs_t or obs_local_t not 16-byte aligned;
 *   2. the params' own: LMAZE_E_NULL params; LMAZE_E_VARIANT an unknown variant; LMAZE_E_GRID; LMAZE_E_LAYOUT n_layouts or
 *      launch_hint;
 *   3. LMAZE_E_VARIANT anything but v5/v6;
 *   4. LMAZE_E_COUNT T < 0 or n outside [0, LMAZE_MAX_ENVS], then controller_key outside {0, 1};
 *   5. T == 0 or n == 0 returns 0 with nothing read;
 *   6. LMAZE_E_NULL a required pointer (layouts, bufs and its members as for lmaze_v5_hier_step, controller, planner), then
 *      LMAZE_E_ALIGN as lmaze_foveal_step.
 * lmaze_foveal_rollout_policy and lmaze_foveal_rollout_sample keep refusing v5/v6.
 * launch_hint bits 0-3, 4-7 and 8-9 as in lmaze_foveal_rollout; they never change results.
 */
int lmaze_v5_rollout_policy(const LmazeFovealParams* params, const uint8_t* layouts, const uint8_t* controller,
                            int32_t controller_key, uint32_t epsilon_u32, const uint8_t* planner,
                            uint32_t planner_epsilon_u32, int32_t T, const LmazeFovealBuffers* bufs, int64_t n, uint64_t seed,
                            uint64_t epoch, int64_t env_base, float* reward_t, uint8_t* done_t, float* foveal_reward_t,
                            uint8_t* foveal_done_t, int32_t* actions_t, int32_t* key_t, int32_t* goals_t, int32_t* goal_key_t,
                            float* obs_t, float* obs_local_t, int32_t obs_every, void* stream);

/* As lmaze_describe_foveal_rollout_policy, for lmaze_v5_rollout_policy with this controller_key and obs_every (0: no recording):
 * "foveal_hier_policy_kernel<v5, 32, 18, obs_t> controller=lds planner=lds T=24 grid=...".  LMAZE_E_NULL text_host NULL or
 * len < 1, then the entry point's refusals 1-4 in their order (obs_every > 0 stands for a given obs_t); an empty line for
 * T == 0 or n == 0.  Nothing is queued or dereferenced. */
int lmaze_describe_v5_rollout_policy(const LmazeFovealParams* params, int64_t n, int32_t T, int32_t controller_key,
                                     int32_t obs_every, char* text_host, int32_t len);

/*
 * SAMPLING closed-loop two-level rollout (v5, v6): lmaze_v5_rollout_policy with a categorical planner and a categorical
 * controller instead of the epsilon-greedy ones -- the form that produces policy-gradient, actor-critic and Boltzmann data for
 * both levels in one launch.  Replaces the user loop of T x (two row gathers, two compare-sums, lmaze_v5_hier_step).  The
 * arguments of lmaze_v5_rollout_policy with `controller, epsilon_u32, planner, planner_epsilon_u32` replaced by
 *   controller_thresholds   const uint32_t*, 16-byte aligned, uint32[keys, 4]: c0, c1, c2 and a reserved word per controller key
 *                           (the grid envs' and v1's format; the reserved word is loaded with the rest and ignored); keys =
 *                           100 for controller_key 0 "offset", 100 L G G for controller_key 1 "cell"
 *   planner_thresholds      const uint32_t*, 16-byte aligned, uint32[L G G, 24]: c0 .. c23 per planner key (the v2/v4 format)
 * Env i (global index e = env_base + i) at step t, ep = epoch + t, gd / ld its done / foveal_done ON ENTRY:
 *   1. r = the exploration draw of lmaze_rollout_policy -- Philox4x32-10(counter (e_lo, e_hi, ep_lo, ep_hi ^ 0x80000000), key
 *      (seed_lo, seed_hi)) -- drawn on every env-step; only r.x and r.z are used;
 *   2. gd: the reset of lmaze_v5_hier_step, same draw, epoch ep (v5:104-150);
 *   3. gd | ld: the planner steps.  kp = the planner key of lmaze_v5_rollout_policy (step 3 there) of the state after that
 *      reset; g = sum over k < 24 of (r.z >= planner_thresholds[kp][k]), unsigned compares; then plannerStep(g) (v5:158-182).
 *      g is always in 0..24, so no plannerStep is ever skipped.  goals_t[t,i] = g, goal_key_t[t,i] = kp; where no plannerStep
 *      was due both are -1;
 *   4. the controller key kc exactly as in lmaze_v5_rollout_policy, steps 4-5: d from the state after 3., kc = d or kp' 100 + d;
 *   5. a = sum over k < 3 of (r.x >= controller_thresholds[kc][k]), unsigned compares; then step(a) (v5:187-292).  a is always
 *      in 0..3.  actions_t[t,i] = a, key_t[t,i] = kc, for every env;
 *   6. reward and done rows of both streams, visit map, obs, obs_local and the recorded slots as in lmaze_foveal_rollout_obs.
 * The caller advances its epoch by T.
 * Goal k is taken with probability (c_k - c_(k-1)) / 2^32, c_(-1) = 0, c_24 = 2^32; an action likewise.  Nothing is validated:
 * a row that is not monotone still yields what the sums give (an implementation by binary search is not equivalent).
 * Each table of at most 16 384 bytes (lmaze_rollout_sample's figure) is staged in LDS once per workgroup, on the next 16-byte
 * boundary behind the layout characters, the controller's first: the 1 600-byte offset controller always, a cell-mode
 * controller (1 600 L G G bytes) never, the planner table (96 L G G bytes) for one layout up to 13 x 13 (16 224 B).  A larger
 * one -- the planner table from 14 x 14 on, 155 520 B for the five 18 x 18 layouts -- is read from global memory: the controller
 * row is one 128-bit read, the planner row six, requested together and only by the envs that plan.  This is a rule, not a
 * measurement; lmaze_describe_v5_rollout_sample reports it as controller=lds|global planner=lds|global.
 * No grid size is refused: the row and the recording form exist for any G, at 32, 64 and 128 envs per workgroup.
 * Refused before anything is queued: the refusals of lmaze_v5_rollout_policy, in its order, with the two threshold tables in
 * the place of `controller` and `planner` (step 6: LMAZE_E_NULL a missing table, with the other pointers); a table that is not
 * 16-byte aligned is LMAZE_E_ALIGN, after the alignment refusals of lmaze_foveal_step.
 * lmaze_foveal_rollout_policy and lmaze_foveal_rollout_sample keep refusing v5/v6.
 * launch_hint bits 0-3, 4-7 and 8-9 as in lmaze_foveal_rollout; they never change results.
 */
int lmaze_v5_rollout_sample(const LmazeFovealParams* params, const uint8_t* layouts, const uint32_t* controller_thresholds,
                            int32_t controller_key, const uint32_t* planner_thresholds, int32_t T, const LmazeFovealBuffers* bufs,
                            int64_t n, uint64_t seed, uint64_t epoch, int64_t env_base, float* reward_t, uint8_t* done_t,
                            float* foveal_reward_t, uint8_t* foveal_done_t, int32_t* actions_t, int32_t* key_t, int32_t* goals_t,
                            int32_t* goal_key_t, float* obs_t, float* obs_local_t, int32_t obs_every, void* stream);

/* As lmaze_describe_v5_rollout_policy, for lmaze_v5_rollout_sample:
 * "foveal_hier_sample_kernel<v5, 32, 18, obs_t> controller=lds planner=global T=24 grid=...".  The same refusals and empty
 * lines.  Nothing is queued or dereferenced. */
int lmaze_describe_v5_rollout_sample(const LmazeFovealParams* params, int64_t n, int32_t T, int32_t controller_key,
                                     int32_t obs_every, char* text_host, int32_t len);

/*
 * v6 safeFovealGoal() (v6:505-523): for every env one window cell index 0..24 drawn uniformly from the
 * cells of the 5x5 window around the ball that are not 'W' (the reference rejects on np.random; here
 * Philox keyed by (seed, env_base + i, epoch), index (r*count)>>32 among the accepted cells in
 * row-major order).  out_goal int32[N].
 */
int lmaze_v6_safe_foveal_goal(const LmazeFovealParams* params, const uint8_t* layouts, uint64_t seed,
                              uint64_t epoch, int64_t env_base, const LmazeFovealBuffers* bufs,
                              int32_t* out_goal, int64_t n, void* stream);

/*
 * The xE nearest-neighbour loop on float planes (v1:258-277, v2:197-203, v4:243-249):
 * out[i, c, x*E+xx, y*E+yy] = planes[i, c, x, y].   planes float[N,C,g,g]; out 16-byte aligned.
 */
int lmaze_expand_planes(const float* planes, int32_t channels, int32_t g, int32_t expansion, float* out,
                        int64_t n, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* LMAZE_H_ */
