// lmaze_foveal_defs.h -- what the translation units of the foveal kernels share (lmaze_foveal.hip: the step, reset and
// open-loop rollout kernels; lmaze_foveal_policy.hip, lmaze_foveal_sample.hip, lmaze_hier_policy.hip, lmaze_hier_sample.hip: the closed-loop rollouts): the kernel arguments, the device helpers
// of lmaze_foveal_body.h, and the host-side checks and LDS sizing their launchers use (the one plan of every foveal launch:
// lmaze_foveal_launch.h).  Not part of the C ABI.
#ifndef LMAZE_FOVEAL_DEFS_H_
#define LMAZE_FOVEAL_DEFS_H_

#include "lmaze_common.h"
#include "lmaze_visit.h"
#include "lmaze_foveal_select.h"
#include "lmaze_foveal_sample.h"
#include "lmaze_hier_select.h"
#include "lmaze_hier_sample.h"

// Timing decomposition (tools/foveal_decompose.py): a build with -DLMAZE_EXPERIMENT -- never the shipped
// one -- reads bits 16-23 of launch_hint as switches that turn phases off (results are garbage then; only the time
// counts): 1 no set-up, 2 plain instead of non-temporal observation stores, 4 no observation stores, 8 no phase 1,
// 16 stores as interleaved 4-KiB pieces, 32 no visit-map phase, 64 / 128 non-temporal visit-map stores / loads.
#ifdef LMAZE_EXPERIMENT
#define LMAZE_WARM_V4(args) ((((args).p.launch_hint >> 16) & 1024) != 0)
#define LMAZE_XP(args, mask) ((((args).p.launch_hint >> 16) & (mask)) != 0)   // round 3: 256 no per-cell work on gathered tiles, 512 no "previous" window tiles
#else
#define LMAZE_WARM_V4(args) false
#define LMAZE_XP(args, mask) false
#endif

namespace lmaze {

constexpr int FOV = LMAZE_FOVEA;
constexpr int W25 = FOV * FOV;

enum FovealMode { FM_STEP = 0, FM_RESET = 1, FM_SETGOAL = 2, FM_PLANNER = 3 };

struct FovealArgs {
    LmazeFovealParams p;
    LmazeFovealBuffers b;
    const uint8_t* layouts;
    const int32_t* action;  // step: action ids; setgoal: ij[N,2]
    const int32_t* goal2;   // v5 two-level step: planner goals (plannerStep of the envs that enter with localDone / done)
    const uint8_t* mask;
    int64_t n;
    int32_t place;
    uint64_t seed, epoch;
    int64_t env_base;
    const uint64_t* epoch_in;  // fused auto-reset from a captured graph: device-resident epoch (lmaze_common.h)
    uint64_t* epoch_out;
    int32_t nt;             // non-temporal observation stores (set by the launcher)
    int32_t auto_reset;     // step: an env whose done flag is set on entry is reset first (v1, v2, v4)
    LaunchInfo* info;       // host pointer; non-null: describe the launch instead of queueing it (lmaze_describe_foveal_step)
};

// The one-launch rollout (foveal_rollout_kernel, lmaze_foveal_rollout): T steps of one chunk of envs before the next
// chunk; step t reads action row t (and planner-goal row t) of the int32[T,N] tensors in FovealArgs and draws its
// resets with epoch + t.  Row t of the trajectory outputs (nullable) gets every env's reward / done after step t.
struct FovealRoll {
    int32_t T;
    float* reward_t;        // [T,N] reward
    uint8_t* done_t;        // [T,N] done
    float* freward_t;       // [T,N] foveal_reward (v1, v5/v6)
    uint8_t* fdone_t;       // [T,N] foveal_done (v1, v5/v6)
};

// The recording rollout (lmaze_foveal_rollout_obs): foveal_rollout_kernel's overload for this type runs with REC = true.
// Step t stores its observation (v5/v6: and, when obs_local_t is given, its local observation) into slot j of the
// caller's tensors when t = (j + 1) every - 1, beside the running obs / obs_local it writes every step.
struct FovealRollObs : FovealRoll {
    float* obs_t;           // [T / every, N, C, 5, 5] or null (no slot)
    float* obs_local_t;     // [T / every, N, 4, 5, 5] or null (v5/v6)
    int32_t every;          // k >= 1
};

// The slots step t fills at this workgroup's first env, or null; the plain rollout has none.  Uniform.
__device__ __forceinline__ float* roll_slot(const FovealRoll&, int64_t, int64_t, int, int) { return nullptr; }
__device__ __forceinline__ float* roll_slot(const FovealRollObs& ro, int64_t n, int64_t base, int t, int per) {
    if (ro.obs_t == nullptr || (t + 1) % ro.every != 0) return nullptr;
    return ro.obs_t + ((size_t)((t + 1) / ro.every - 1) * n + base) * per;
}
__device__ __forceinline__ float* roll_lslot(const FovealRoll&, int64_t, int64_t, int) { return nullptr; }
__device__ __forceinline__ float* roll_lslot(const FovealRollObs& ro, int64_t n, int64_t base, int t) {
    if (ro.obs_local_t == nullptr || (t + 1) % ro.every != 0) return nullptr;
    return ro.obs_local_t + ((size_t)((t + 1) / ro.every - 1) * n + base) * (4 * W25);
}
__device__ __forceinline__ void roll_store4(const FovealRoll&, float4*, const float*) {}
__device__ __forceinline__ void roll_store4(const FovealRollObs&, float4* p, const float* v) {
    *p = make_float4(v[0], v[1], v[2], v[3]);
}

// The closed-loop rollout (lmaze_foveal_rollout_policy, lmaze_foveal_policy.hip): the tabular epsilon-greedy policy that
// stands where the action tensor stood.  The body is compiled with its POL switch on for the two types below and reads
// ro.pol.
struct FovealPol {
    const uint8_t* table;   // uint8[L*G*G]: the greedy action id of every key
    uint32_t epsilon;       // min(floor(eps * 2^32), 2^32 - 1); 0 draws nothing
    int32_t in_lds;         // the table is staged in LDS behind the layout characters (L*G*G <= 8192), else read from global memory
    int32_t* actions_t;     // [T,N] or null: the action every env took
    int32_t* key_t;         // [T,N] or null: the key it was looked up with
};
struct FovealRollPol : FovealRoll { FovealPol pol; };
struct FovealRollObsPol : FovealRollObs { FovealPol pol; };
// The action of an env in state (lid, bx, by): key -> table -> epsilon mix with the draw r (lmaze_foveal_select.h), and
// element `row` of the action and key rows, stored here for every env, skipped ones included (nothing of them stays live
// through the rest of phase 1).  The staged and the global table are read through pointers of their own address spaces:
// as two generic loads they merge into one flat load of a selected pointer (lmaze_step.hip policy_act).
__device__ __forceinline__ int foveal_pol_action(const FovealPol& pol, bool staged, const uint8_t* lds_table, int lid, int bx, int by,
                                                 int G, int L, int A, const uint4& r, int64_t row) {
    typedef const __attribute__((address_space(3))) uint8_t* lds_bytes;
    typedef const __attribute__((address_space(1))) uint8_t* global_bytes;
    const int key = lmaze_foveal_key(lid, bx, by, G, L);
    const int greedy = staged ? (int)((lds_bytes)lds_table)[key] : (int)((global_bytes)pol.table)[key];
    const int act = lmaze_foveal_choose(greedy, r.x, r.y, pol.epsilon, A);
    if (pol.actions_t) pol.actions_t[row] = act;
    if (pol.key_t) pol.key_t[row] = key;
    return act;
}
constexpr int kFovealPolicyLds = 8192;   // bytes of table up to which it is staged in LDS (a rule, not a measurement)
// rec false: the plain form, the recording members of ro unread (lmaze_foveal_launch.h launch_foveal_rollout_sliced)
hipError_t launch_foveal_rollout_closed(const FovealArgs& a, const FovealRollObsPol& ro, bool rec, hipStream_t s);

// The sampling closed-loop rollout (lmaze_foveal_rollout_sample, lmaze_foveal_sample.hip): a categorical table policy, one
// row of cumulative thresholds per key -- uint32[4] for v1 (c0, c1, c2, reserved: the grid envs' format), uint32[24] for
// v2/v4 -- and one draw word per env-step compared against them (lmaze_foveal_sample.h).  The body is compiled with POL = 2
// for the two types below and reads ro.smp.
struct FovealSmp {
    const uint32_t* table;  // uint32[L*G*G, 4 or 24], 16-byte aligned
    int32_t in_lds;         // the table is staged in LDS behind the layout characters (at most kFovealSampleLds bytes), else read from global memory
    int32_t* actions_t;     // [T,N] or null: the action every env took
    int32_t* key_t;         // [T,N] or null: the key its row was looked up with
};
struct FovealRollSmp : FovealRoll { FovealSmp smp; };
struct FovealRollObsSmp : FovealRollObs { FovealSmp smp; };
typedef uint32_t foveal_row4_t __attribute__((ext_vector_type(4)));
// The whole table into LDS, 16 bytes per lane and turn (n16 pieces); the caller's barrier follows.
__device__ __forceinline__ void stage_thresholds(uint32_t* lds_table, const uint32_t* table, int n16, int tid) {
    typedef __attribute__((address_space(3))) foveal_row4_t* lds_rows;
    typedef const __attribute__((address_space(1))) foveal_row4_t* global_rows;
    for (int i = tid; i < n16; i += LMAZE_BLOCK) ((lds_rows)lds_table)[i] = ((global_rows)table)[i];
}
// The action of an env in state (lid, bx, by) from the draw word r: key -> the key's row, one (v1) or six 128-bit reads
// requested together, none depending on another -> the sum of compares, and element `row` of the action and key rows.  The
// staged and the global table are read through pointers of their own address spaces (foveal_pol_action).  v1 reads its
// reserved word with the rest and keeps it to the end, so that the row stays one 128-bit read.
template <bool V1>
__device__ __forceinline__ int foveal_smp_action(const FovealSmp& smp, bool staged, const uint32_t* lds_table, int lid, int bx, int by,
                                                 int G, int L, uint32_t r, int64_t row) {
    typedef const __attribute__((address_space(3))) foveal_row4_t* lds_rows;
    typedef const __attribute__((address_space(1))) foveal_row4_t* global_rows;
    constexpr int Q = V1 ? 1 : 6, NC = V1 ? 3 : 24;
    const int key = lmaze_foveal_key(lid, bx, by, G, L);
    foveal_row4_t q[Q];
    if (staged) {
#pragma unroll
        for (int j = 0; j < Q; ++j) q[j] = ((lds_rows)lds_table)[key * Q + j];
    } else {
#pragma unroll
        for (int j = 0; j < Q; ++j) q[j] = ((global_rows)smp.table)[(size_t)key * Q + j];
    }
    uint32_t c[Q * 4];
#pragma unroll
    for (int j = 0; j < Q; ++j) { c[4 * j] = q[j].x; c[4 * j + 1] = q[j].y; c[4 * j + 2] = q[j].z; c[4 * j + 3] = q[j].w; }
    const int act = lmaze_foveal_sample_action(c, NC, r);
    if (V1) asm volatile("" ::"v"(c[3]));
    if (smp.actions_t) smp.actions_t[row] = act;
    if (smp.key_t) smp.key_t[row] = key;
    return act;
}
constexpr int kFovealSampleLds = 16384;   // bytes of thresholds up to which they are staged in LDS: lmaze_rollout_sample's figure
hipError_t launch_foveal_rollout_closed(const FovealArgs& a, const FovealRollObsSmp& ro, bool rec, hipStream_t s);

// The closed-loop TWO-LEVEL rollout of v5/v6 (lmaze_v5_rollout_policy, lmaze_hier_policy.hip): two uint8 tables, the planner's
// keyed by (layout row, ball) and the controller's by the foveal goal's offset from the ball (and, controller_key 1, the
// planner key as well), each mixed with two words of one exploration draw (lmaze_hier_select.h).  The body is compiled with
// POL = 3 for the two types below and reads ro.hier.
struct FovealHier {
    const uint8_t* controller;   // uint8[100] or uint8[100*L*G*G]: the greedy action id of every controller key
    const uint8_t* planner;      // uint8[L*G*G]: the greedy goal id of every planner key
    uint32_t epsilon;            // controller: min(floor(eps * 2^32), 2^32 - 1)
    uint32_t planner_epsilon;    // planner: likewise; nothing is drawn when both are 0
    int32_t controller_key;      // 0 offset, 1 cell
    int32_t in_lds;              // bit 0: the controller table is staged in LDS behind the layout characters, bit 1: the planner table, behind it
    int32_t* actions_t;          // [T,N] or null: the action every env took
    int32_t* key_t;              // [T,N] or null: the controller key it was looked up with
    int32_t* goals_t;            // [T,N] or null: the goal of every env that planned, -1 elsewhere
    int32_t* goal_key_t;         // [T,N] or null: the planner key it was looked up with, -1 elsewhere
};
struct FovealRollHier : FovealRoll { FovealHier hier; };
struct FovealRollObsHier : FovealRollObs { FovealHier hier; };
constexpr int kHierControllerStaged = 1, kHierPlannerStaged = 2;
__host__ __device__ __forceinline__ int hier_controller_bytes(int controller_key, int L, int G) {
    return controller_key ? LMAZE_HIER_OFFSETS * L * G * G : LMAZE_HIER_OFFSETS;
}
// Staging a table of `bytes` bytes: its first two dwords per lane are requested here (beside the layout loads, before the
// row masks are built) ...
__device__ __forceinline__ void hier_request(const uint8_t* table, int bytes, bool dwords, int tid, uint32_t (&w)[2]) {
    w[0] = w[1] = 0u;
    if (!dwords) return;
#pragma unroll
    for (int j = 0; j < 2; ++j)
        if (tid + j * LMAZE_BLOCK < bytes >> 2) w[j] = reinterpret_cast<const uint32_t*>(table)[tid + j * LMAZE_BLOCK];
}
// ... and stored here, with whatever lies past 2 KiB; a table that is not whole aligned dwords goes byte by byte.  The
// caller's barrier follows.
__device__ __forceinline__ void hier_stage(uint8_t* lds_table, const uint8_t* table, int bytes, bool dwords, int tid, const uint32_t (&w)[2]) {
    if (dwords) {
#pragma unroll
        for (int j = 0; j < 2; ++j)
            if (tid + j * LMAZE_BLOCK < bytes >> 2) reinterpret_cast<uint32_t*>(lds_table)[tid + j * LMAZE_BLOCK] = w[j];
        for (int i = tid + 2 * LMAZE_BLOCK; i < bytes >> 2; i += LMAZE_BLOCK)
            reinterpret_cast<uint32_t*>(lds_table)[i] = reinterpret_cast<const uint32_t*>(table)[i];
    } else {
        for (int i = tid; i < bytes; i += LMAZE_BLOCK) lds_table[i] = table[i];
    }
}
// One byte of a table: the staged and the global side are read through pointers of their own address spaces (foveal_pol_action).
__device__ __forceinline__ int hier_table_byte(bool staged, const uint8_t* lds_table, const uint8_t* table, int key) {
    typedef const __attribute__((address_space(3))) uint8_t* lds_bytes;
    typedef const __attribute__((address_space(1))) uint8_t* global_bytes;
    return staged ? (int)((lds_bytes)lds_table)[key] : (int)((global_bytes)table)[key];
}
// The goal of an env that plans in state (lid, bx, by): planner key -> table -> mix with the draw words r.z / r.w, and element
// `row` of the goal and goal-key rows, stored here where they are produced.
__device__ __forceinline__ int hier_plan_goal(const FovealHier& h, const uint8_t* lds_table, int lid, int bx, int by, int G, int L,
                                              uint32_t rz, uint32_t rw, int64_t row) {
    const int kp = lmaze_hier_planner_key(lid, bx, by, G, L);
    const int g = lmaze_hier_goal(hier_table_byte((h.in_lds & kHierPlannerStaged) != 0, lds_table, h.planner, kp), rz, rw, h.planner_epsilon);
    if (h.goals_t) h.goals_t[row] = g;
    if (h.goal_key_t) h.goal_key_t[row] = kp;
    return g;
}
// ... and of an env that does not: both rows are -1.
__device__ __forceinline__ void hier_no_goal(const FovealHier& h, int64_t row) {
    if (h.goals_t) h.goals_t[row] = -1;
    if (h.goal_key_t) h.goal_key_t[row] = -1;
}
// The action of an env whose state after the plannerStep is (lid, bx, by, fgx, fgy): controller key -> table -> mix with the
// draw words r.x / r.y, and element `row` of the action and key rows.
__device__ __forceinline__ int hier_act(const FovealHier& h, const uint8_t* lds_table, int lid, int bx, int by, int fgx, int fgy, int G,
                                        int L, uint32_t rx, uint32_t ry, int64_t row) {
    const int d = lmaze_hier_offset(fgx, fgy, bx, by);
    const int kc = lmaze_hier_controller_key(h.controller_key, h.controller_key ? lmaze_hier_planner_key(lid, bx, by, G, L) : 0, d);
    const int act = lmaze_hier_action(hier_table_byte((h.in_lds & kHierControllerStaged) != 0, lds_table, h.controller, kc), rx, ry, h.epsilon);
    if (h.actions_t) h.actions_t[row] = act;
    if (h.key_t) h.key_t[row] = kc;
    return act;
}
// rec false: the row form, the recording members of ro unread (lmaze_foveal_launch.h launch_foveal_rollout_sliced)
hipError_t launch_foveal_rollout_closed(const FovealArgs& a, const FovealRollObsHier& ro, bool rec, hipStream_t s);

// The SAMPLING closed-loop two-level rollout of v5/v6 (lmaze_v5_rollout_sample, lmaze_hier_sample.hip): both levels draw from
// categorical tables -- the controller's one row uint32[4] per controller key (c0, c1, c2, reserved: the grid envs' and v1's
// format), the planner's one row uint32[24] per planner key (the v2/v4 format) -- compared against the words r.x and r.z of
// ONE draw per env-step (lmaze_hier_sample.h).  The body is compiled with POL = 4 for the two types below and reads ro.hsmp.
struct FovealHierSmp {
    const uint32_t* controller;  // uint32[100, 4] or uint32[100*L*G*G, 4], 16-byte aligned
    const uint32_t* planner;     // uint32[L*G*G, 24], 16-byte aligned
    int32_t controller_key;      // 0 offset, 1 cell
    int32_t in_lds;              // kHierControllerStaged: the controller table is staged in LDS on the next 16-byte boundary behind the
                                 // layout characters; kHierPlannerStaged: the planner table, behind it
    int32_t* actions_t;          // [T,N] or null: the action every env took
    int32_t* key_t;              // [T,N] or null: the controller key its row was looked up with
    int32_t* goals_t;            // [T,N] or null: the goal of every env that planned, -1 elsewhere
    int32_t* goal_key_t;         // [T,N] or null: the planner key its row was looked up with, -1 elsewhere
};
struct FovealRollHierSmp : FovealRoll { FovealHierSmp hsmp; };
struct FovealRollObsHierSmp : FovealRollObs { FovealHierSmp hsmp; };
__host__ __device__ __forceinline__ int64_t hier_sample_controller_bytes(int controller_key, int L, int G) {
    return (int64_t)lmaze_hier_sample_controller_keys(controller_key, L, G) * (LMAZE_HIER_SAMPLE_CROW * 4);
}
__host__ __device__ __forceinline__ int64_t hier_sample_planner_bytes(int L, int G) { return (int64_t)L * G * G * (LMAZE_HIER_SAMPLE_PROW * 4); }
// A key's row, Q 128-bit reads requested together, the staged and the global side through pointers of their own address
// spaces (foveal_smp_action).
template <int Q>
__device__ __forceinline__ void hier_smp_row(bool staged, const uint32_t* lds_table, const uint32_t* table, int key, uint32_t (&c)[Q * 4]) {
    typedef const __attribute__((address_space(3))) foveal_row4_t* lds_rows;
    typedef const __attribute__((address_space(1))) foveal_row4_t* global_rows;
    foveal_row4_t q[Q];
    if (staged) {
#pragma unroll
        for (int j = 0; j < Q; ++j) q[j] = ((lds_rows)lds_table)[key * Q + j];
    } else {
#pragma unroll
        for (int j = 0; j < Q; ++j) q[j] = ((global_rows)table)[(size_t)key * Q + j];
    }
#pragma unroll
    for (int j = 0; j < Q; ++j) { c[4 * j] = q[j].x; c[4 * j + 1] = q[j].y; c[4 * j + 2] = q[j].z; c[4 * j + 3] = q[j].w; }
}
// The goal of an env that plans in state (lid, bx, by): planner key -> the key's row, six 128-bit reads in one group -> the sum
// of compares against r.z, and element `row` of the goal and goal-key rows, stored here where they are produced.
__device__ __forceinline__ int hier_smp_goal(const FovealHierSmp& h, const uint32_t* lds_table, int lid, int bx, int by, int G, int L,
                                             uint32_t rz, int64_t row) {
    const int kp = lmaze_hier_planner_key(lid, bx, by, G, L);
    uint32_t c[LMAZE_HIER_SAMPLE_PROW];
    hier_smp_row<LMAZE_HIER_SAMPLE_PROW / 4>((h.in_lds & kHierPlannerStaged) != 0, lds_table, h.planner, kp, c);
    const int g = lmaze_hier_sample_goal(c, rz);
    if (h.goals_t) h.goals_t[row] = g;
    if (h.goal_key_t) h.goal_key_t[row] = kp;
    return g;
}
// ... and of an env that does not: both rows are -1.
__device__ __forceinline__ void hier_smp_no_goal(const FovealHierSmp& h, int64_t row) {
    if (h.goals_t) h.goals_t[row] = -1;
    if (h.goal_key_t) h.goal_key_t[row] = -1;
}
// The action of an env whose state after the plannerStep is (lid, bx, by, fgx, fgy): controller key -> the key's row, one
// 128-bit read (the reserved word is read with the rest and kept to the end, foveal_smp_action) -> the sum of compares against
// r.x, and element `row` of the action and key rows.
__device__ __forceinline__ int hier_smp_act(const FovealHierSmp& h, const uint32_t* lds_table, int lid, int bx, int by, int fgx, int fgy,
                                            int G, int L, uint32_t rx, int64_t row) {
    const int d = lmaze_hier_offset(fgx, fgy, bx, by);
    const int kc = lmaze_hier_controller_key(h.controller_key, h.controller_key ? lmaze_hier_planner_key(lid, bx, by, G, L) : 0, d);
    uint32_t c[LMAZE_HIER_SAMPLE_CROW];
    hier_smp_row<1>((h.in_lds & kHierControllerStaged) != 0, lds_table, h.controller, kc, c);
    const int act = lmaze_hier_sample_action(c, rx);
    asm volatile("" ::"v"(c[3]));
    if (h.actions_t) h.actions_t[row] = act;
    if (h.key_t) h.key_t[row] = kc;
    return act;
}
// rec false: the row form, the recording members of ro unread (lmaze_foveal_launch.h launch_foveal_rollout_sliced)
hipError_t launch_foveal_rollout_closed(const FovealArgs& a, const FovealRollObsHierSmp& ro, bool rec, hipStream_t s);

struct EnvRec {           // one env after its transition (registers only; phase 1 turns it into plane masks)
    int16_t cx, cy;       // centre of the current window (ball after the move)
    int16_t px, py;       // centre of the "previous" window
    int16_t gx, gy;       // goal (v2/v4) or foveal goal (v1 local view)
    int16_t lid;          // row of the layout table
    int16_t action;       // v2/v4 action plane (-1: none); v1: 1 = local view, 0 = global view
    int32_t skip;         // env untouched by this call: neither state nor obs are written
    int32_t flat;         // v1 local view: flat index of the one-hot goal (numpy wrap applied), -1 none
    int16_t b0x, b0y;     // v5/v6 local observation: ball, previous ball, fovea_1 (v5:364-365)
    int16_t b1x, b1y;
    int16_t f1x, f1y;
    int16_t upd;          // v5/v6: localDone -> this call halves the visit map (v5:313-318)
    int16_t pad;
};

// Placement on row masks.  rows[x] has bit y set when interior cell (x, y) is accepted; accepted cells are
// ranked in row-major order (the order of the reference's own scan over the grid).

// accepted cells of the goal and of the ball mask, one pass.  Unrolled by 4 and no more: the loop is a chain of LDS round
// trips in a lane that a whole wave waits for (some lane of most waves resets at steady state), so it wants several
// reads in flight, but with G known at compile time a FULL unroll keeps a layout's row masks live and the fused-reset
// instantiation then needs 115 VGPRs (4 waves per SIMD instead of 7) for the whole kernel
template <int U>
__device__ __forceinline__ void mask_counts(const uint64_t* goal_rows, const uint64_t* ball_rows, int G, int& cg, int& cb) {
    cg = 0; cb = 0;
#pragma unroll U
    for (int x = 1; x <= G - 2; ++x) { cg += __popcll(goal_rows[x]); cb += __popcll(ball_rows[x]); }
}

// k-th accepted cell (0-based) as x*G + y, or -1, of the mask with cell `hole` (x*G + y; negative: none) taken out.
// No early exit, so that the row reads pipeline (see mask_counts).  The hole is tested as "hole - x*G in [0, G)" so that
// nothing but the cell index itself stays live across the loop.
template <int U>
__device__ __forceinline__ int mask_kth(const uint64_t* rows, int G, int k, int hole) {
    int xr = -1, kk = 0, acc = 0;
#pragma unroll U
    for (int x = 1; x <= G - 2; ++x) {
        uint64_t m = rows[x];
        const unsigned hy = (unsigned)(hole - x * G);
        if (hy < (unsigned)G) m &= ~(1ull << hy);
        const int c = __popcll(m);
        if (xr < 0 && k < acc + c) { xr = x; kk = k - acc; }
        acc += c;
    }
    if (xr < 0) return -1;
    uint64_t m = rows[xr];
    const unsigned hy = (unsigned)(hole - xr * G);
    if (hy < (unsigned)G) m &= ~(1ull << hy);
    uint32_t h = (uint32_t)m;
    int base = 0;
    const int cl = __popc(h);
    if (kk >= cl) { kk -= cl; h = (uint32_t)(m >> 32); base = 32; }
    for (; kk > 0; --kk) h &= h - 1;
    return xr * G + base + (__ffs((int)h) - 1);
}

// reset() placement of v2/v4/v5/v6 on one layout (v2:277-296): goal uniform over interior cells that are
// not 'W' and not 'S'; ball uniform over interior cells that are not 'W', not 'X' and not the goal.  Accepted cells
// are ranked row-major (the order of the reference's own scan); "not the goal" = the goal's bit taken out of the
// ball mask, which leaves the ranking of every other cell as the reference's list has it.
template <int U>
__device__ __forceinline__ void place_goal_ball(const uint64_t* goal_rows, const uint64_t* ball_rows, int G, uint4 d,
                                                int& goal_cell, int& ball_cell) {
    goal_cell = -1;
    ball_cell = -1;
    int cg, cb;
    mask_counts<U>(goal_rows, ball_rows, G, cg, cb);
    if (cg > 0) goal_cell = mask_kth<U>(goal_rows, G, (int)__umulhi(d.x, (uint32_t)cg), -1);
    if (goal_cell >= 0 && ((ball_rows[goal_cell / G] >> (goal_cell % G)) & 1ull)) --cb;   // a 'B' goal cell leaves the ball's list
    if (cb > 0) ball_cell = mask_kth<U>(ball_rows, G, (int)__umulhi(d.y, (uint32_t)cb), goal_cell);
}

// numpy index semantics on an axis of 5: -5..-1 wrap, anything else outside 0..4 raises (-> -1)
__device__ __forceinline__ int wrap5(int i) {
    if (i >= 0 && i < FOV) return i;
    if (i < 0 && i >= -FOV) return i + FOV;
    return -1;
}

// 25-bit mask (bit 5*i+j) of a 5x5 window centred on (cx, cy) over a plane given as one 64-bit row
// mask per layout row (bit y = cell (x, y) is set); cells outside the array read 0
__device__ __forceinline__ uint32_t window_bits(const uint64_t* rows, int G, int cx, int cy) {
    uint32_t m = 0;
    const int y0 = cy - 2;
#pragma unroll
    for (int i = 0; i < FOV; ++i) {
        const int x = cx - 2 + i;
        const uint64_t b = (x >= 0 && x < G) ? rows[x] : 0ull;
        const uint32_t w = (uint32_t)(y0 >= 0 ? (b >> y0) : (b << -y0)) & 31u;
        m |= w << (FOV * i);
    }
    return m;
}

// bit of cell (tx, ty) inside the window centred on (cx, cy), 0 if it is outside the window
__device__ __forceinline__ uint32_t onehot_bits(int tx, int ty, int cx, int cy) {
    const int i = tx - cx + 2, j = ty - cy + 2;
    return (i >= 0 && i < FOV && j >= 0 && j < FOV) ? (1u << (FOV * i + j)) : 0u;
}

// OR the 25-bit plane m into a bit string at bit offset off (LDS atomics: neighbouring envs share words)
__device__ __forceinline__ void put_bits(uint32_t* bits, int off, uint32_t m) {
    const int w = off >> 5, sh = off & 31;
    atomicOr(&bits[w], m << sh);
    if (sh > 32 - W25) atomicOr(&bits[w + 1], m >> (32 - sh));
}

// 16 bytes per lane from global memory straight into LDS (global_load_lds_dwordx4, gfx950): no register destination.
// `lds_wave_base` is WAVE-UNIFORM: lane l's bytes land at lds_wave_base + 16 l whatever the exec mask.
__device__ __forceinline__ void lds_dma16(const uint32_t* src, uint32_t* lds_wave_base) {
    typedef __attribute__((address_space(1))) void gvoid;
    typedef __attribute__((address_space(3))) void lvoid;
    __builtin_amdgcn_global_load_lds((gvoid*)src, (lvoid*)lds_wave_base, 16, 0, 0);
}

// four consecutive floats (0.0f / 1.0f) from nibble q of a bit string
__device__ __forceinline__ void nibble_floats(const uint32_t* bits, int q, float (&v)[4]) {
    const uint32_t nib = bits[q >> 3] >> ((q & 7) << 2);
#pragma unroll
    for (int k = 0; k < 4; ++k) v[k] = __uint_as_float((0u - ((nib >> k) & 1u)) & 0x3f800000u);
}

// The visit map in its clock-relative frame: the bit-pattern arithmetic lives in lmaze_visit.h (shared with the host-side
// property test of the CPU suite); here only the tile geometry.
constexpr int VISIT_BIAS = LMAZE_VISIT_BIAS, VISIT_RENORM = LMAZE_VISIT_RENORM;
constexpr int VT = 4;                // tile side; a tile is 16 floats = 64 bytes
// Behind an env batch's tiles the visit buffer holds one record of VPC words per env: the true values of the 5x5 window
// the observation shows as "previous" (retStatelast: v4:239,259, v5:322-346), word 25 = a tag naming the centre they
// belong to.  v5/v6 show that window unchanged for up to ten steps and v4 shows last step's current window, so it is
// kept as 112 contiguous bytes instead of being gathered from up to four more tiles every step.
constexpr int VPC = 28;
// Which centre the record belongs to rides in the upper bits of the env's visit_clock word (bits 0-7 the clock, bit 8
// "record valid", bits 9-15 / 16-22 the centre): one coalesced load in phase 1 tells whether the record serves this call.
__host__ __device__ __forceinline__ int visit_tag(int x, int y) { return 0x100 | ((x & 0x7f) << 9) | ((y & 0x7f) << 16); }

__host__ __device__ __forceinline__ int visit_tiles(int G) { return (G + VT - 1) / VT; }
__device__ __forceinline__ uint32_t visit_true(uint32_t bits, int E) { return lmaze_visit_true(bits, E); }
__device__ __forceinline__ uint32_t visit_add(uint32_t bits, int E) { return lmaze_visit_add(bits, E); }

// GT = grid side known at compile time (14 and 18, the reference's sizes; 0: read it from the params):
// the visit-map stream divides by G for every cell, which is only cheap with a constant
// AR = fused auto-reset compiled in (a separate instantiation: the extra state it threads through the
// visit-map stream costs the plain step 20 % when it is only a run-time flag)
#ifndef LMAZE_WIN_SUB
#define LMAZE_WIN_SUB 64    // envs whose window rows one pass of phase 2 holds in registers
#endif

// ---- host side: LDS sizing and the checks every foveal entry point starts with ----
constexpr size_t kFovealStreamBytes = (size_t)192 << 20;   // observations larger than this are streamed (non-temporal stores)

// LDS one workgroup may ask for on this device (160 KiB on gfx950), queried once
static inline size_t lds_limit() {
    static size_t limit = 0;
    if (limit == 0) {
        int dev = 0, v = 0;
        if (hipGetDevice(&dev) == hipSuccess && hipDeviceGetAttribute(&v, hipDeviceAttributeMaxSharedMemoryPerBlock, dev) == hipSuccess && v > 0)
            limit = (size_t)v;
        else
            limit = 64 * 1024;
    }
    return limit;
}

// planes of a variant's observation
static inline int foveal_channels(int variant) { return variant == LMAZE_VARIANT_V1 ? 4 : (variant == LMAZE_VARIANT_V2 ? 5 : 7); }

// dynamic LDS of foveal_body for epb envs per workgroup; variant: the kernels' (v5 for v6)
static inline size_t foveal_lds(int variant, const LmazeFovealParams& p, int epb) {
    const int cells = p.grid * p.grid;
    const int L = variant == LMAZE_VARIANT_V1 ? 1 : p.n_layouts;
    // obs bit string 32 B + obs_local bit string 16 B + centres 8 B + flags 4 B + reset centre 4 B per env, row masks, layout characters, visit samples
    size_t lds = (size_t)epb * 64 + (3 * (size_t)L * p.grid + 2 * (size_t)p.grid) * 8 + (size_t)((L * cells + 15) & ~15);
    if (variant == LMAZE_VARIANT_V4 || variant == LMAZE_VARIANT_V5)
        lds += (size_t)epb * (2 * W25 * 4 + 8);   // + visit samples, clock, whole-map list
    return lds;
}

// launch_hint bits 0-3 (step and rollout): at most that many workgroups resident per CU, by padding the dynamic LDS
static inline size_t lds_for_cap(size_t lds, int per_cu) {
    if (per_cu >= 1 && per_cu <= 8) {
        const size_t cap = 160 * 1024;
        const size_t want = ((cap / per_cu + cap / (per_cu + 1)) / 2) & ~(size_t)255;   // between the two thresholds
        if (want > lds && want <= lds_limit()) return want;     // per_cu 1 (120 KiB) and 2 (66 KiB) included where the device allows
    }
    return lds;
}

static inline bool foveal_grid_ok(int g) { return g >= FOV && g <= LMAZE_MAX_GRID; }

// The refusals that need only the params, in this order: the variant, the grid side, the number of layouts.  The env count
// and launch_hint's range are calls of their own, because the entry points order them differently (the step family answers
// the count first, the closed-loop rollouts the hint; the describes do not look at the hint).
static inline int check_foveal_params(const LmazeFovealParams* p) {
    if (!p) return LMAZE_E_NULL;
    if (p->variant != LMAZE_VARIANT_V1 && p->variant != LMAZE_VARIANT_V2 && p->variant != LMAZE_VARIANT_V4 &&
        p->variant != LMAZE_VARIANT_V5 && p->variant != LMAZE_VARIANT_V6)
        return LMAZE_E_VARIANT;
    if (!foveal_grid_ok(p->grid)) return LMAZE_E_GRID;
    if (p->n_layouts < 1 || p->n_layouts > LMAZE_MAX_LAYOUTS) return LMAZE_E_LAYOUT;
    return 0;
}
static inline int check_foveal_count(int64_t n) { return n < 0 || n > LMAZE_MAX_ENVS ? LMAZE_E_COUNT : 0; }
static inline int check_foveal_hint(const LmazeFovealParams* p) { return (p->launch_hint & ~0x3ff) ? LMAZE_E_LAYOUT : 0; }

static inline int check_foveal(const LmazeFovealParams* p, const uint8_t* layouts, const LmazeFovealBuffers* b, int64_t n) {
    if (!p || !layouts || !b) return LMAZE_E_NULL;
    int rc = check_foveal_params(p);
    if (!rc) rc = check_foveal_count(n);
#ifndef LMAZE_EXPERIMENT
    if (!rc) rc = check_foveal_hint(p);
#endif
    if (rc) return rc;
    const bool v56 = p->variant == LMAZE_VARIANT_V5 || p->variant == LMAZE_VARIANT_V6;
    if (v56) {
        if (!b->fgoal_xy || !b->foveal_step_count || !b->foveal_reward || !b->foveal_done || !b->visit || !b->ball1_xy ||
            !b->fovea_xy || !b->last_xy || !b->foveal_goal || !b->obs_local)
            return LMAZE_E_NULL;
        if ((uintptr_t)b->obs_local & 15) return LMAZE_E_ALIGN;
    }
    if (!b->ball_xy || !b->step_count || !b->reward || !b->done || !b->obs) return LMAZE_E_NULL;
    if (p->variant == LMAZE_VARIANT_V1 && (!b->fgoal_xy || !b->foveal_step_count || !b->foveal_reward || !b->foveal_done))
        return LMAZE_E_NULL;
    if (p->variant != LMAZE_VARIANT_V1 && (!b->goal_xy || !b->layout_id)) return LMAZE_E_NULL;
    if ((p->variant == LMAZE_VARIANT_V4 || v56) && (!b->visit || !b->visit_clock)) return LMAZE_E_NULL;
    if (((uintptr_t)b->obs & 15) || (b->visit && ((uintptr_t)b->visit & 63))) return LMAZE_E_ALIGN;   // a tile = one 64-byte sector
    return 0;
}

// The draws of an entry that resets or places (seed, epoch, env_base), its fused reset or two-level step (auto_reset) and the
// device-resident epoch words (lmaze_common.h)
struct FovealReset {
    int32_t auto_reset;
    uint64_t seed, epoch;
    int64_t env_base;
    const uint64_t* epoch_in;
    uint64_t* epoch_out;
};
constexpr FovealReset kNoFovealReset{0, 0, 0, 0, nullptr, nullptr};

// b null: a describe, which dereferences nothing -- the launcher fills a.info where it would have queued the kernel
static inline FovealArgs make_foveal_args(const LmazeFovealParams* p, const uint8_t* layouts, const LmazeFovealBuffers* b, int64_t n,
                                          const FovealReset& r = kNoFovealReset) {
    // in FovealArgs' order: action, goal2, mask null, place 0, ..., nt 0, ..., info null
    return FovealArgs{*p, b ? *b : LmazeFovealBuffers{}, layouts, nullptr, nullptr, nullptr, n, 0, r.seed, r.epoch, r.env_base,
                      r.epoch_in, r.epoch_out, 0, r.auto_reset ? 1 : 0, nullptr};
}

}  // namespace lmaze

#endif  // LMAZE_FOVEAL_DEFS_H_
