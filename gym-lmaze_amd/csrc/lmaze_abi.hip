// lmaze_abi.hip -- the extern "C" surface declared in include/lmaze.h: argument checks and
// launches only.  No allocation, no synchronisation, no host-side compute fallback: if the
// launch fails the hipError_t goes back to the caller.
#include <stdio.h>
#include <string.h>

#include "lmaze_common.h"
#include "lmaze_foveal_defs.h"
#include "lmaze_offpolicy.h"


using namespace lmaze;

static int check_params(const LmazeParams* p, int64_t n) {
    if (!p) return LMAZE_E_NULL;
    if (p->grid < 3 || p->grid > LMAZE_MAX_GRID) return LMAZE_E_GRID;
    if (p->layout_mode != LMAZE_LAYOUT_SHARED && p->layout_mode != LMAZE_LAYOUT_PER_ENV) return LMAZE_E_LAYOUT;
    if (n < 0 || n > LMAZE_MAX_ENVS) return LMAZE_E_COUNT;
    return 0;
}

static bool misaligned(const void* p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) != 0; }

// The variants a grid entry takes
enum { TAKES_V0 = 1, TAKES_V3 = 2, TAKES_BOTH = 3 };

// The narrow (uint8) planes: shared layouts and G >= 4 only
static int check_narrow(const LmazeParams* p) {
    if (p->layout_mode != LMAZE_LAYOUT_SHARED) return LMAZE_E_LAYOUT;
    if (p->grid < 4) return LMAZE_E_GRID;                  // a 16-byte store must not span more than two envs
    return 0;
}

// What every grid step and rollout entry judges first, in this order: the params, the variant against what the entry takes
// and, with u8, the narrow planes' own refusals
static int check_grid_params(const LmazeParams* p, int64_t n, int takes, bool u8) {
    const int rc = check_params(p, n);
    if (rc) return rc;
    if (!(p->variant == LMAZE_VARIANT_V0 && (takes & TAKES_V0)) && !(p->variant == LMAZE_VARIANT_V3 && (takes & TAKES_V3)))
        return LMAZE_E_VARIANT;
    return u8 ? check_narrow(p) : 0;
}

// ... and last, the buffers: LMAZE_E_NULL for the layout, ball_xy, goal_xy under v3's rules and the others the entry needs
// (`others`: false if one of them is missing), then LMAZE_E_ALIGN -- ball_xy / goal_xy 8 bytes, the planes 16, the layout 16
// unless the planes are narrow (those kernels read it by bytes), and a closed-loop rollout's table as it says
static int check_buffers(const LmazeParams* p, bool u8, const void* layout, const void* ball_xy, const void* goal_xy, const void* obs,
                         bool others, const void* table = nullptr, uintptr_t table_align = 1) {
    if (!layout || !ball_xy || !others || (p->variant == LMAZE_VARIANT_V3 && !goal_xy)) return LMAZE_E_NULL;
    if (misaligned(ball_xy, 8) || misaligned(goal_xy, 8) || misaligned(obs, 16) || (!u8 && misaligned(layout, 16)) ||
        misaligned(table, table_align))
        return LMAZE_E_ALIGN;
    return 0;
}

// The StepArgs of a grid step or rollout: obs the int32 planes, or with u8 the narrow ones (a.obs8).  v0 keeps no goal_xy,
// v3 no goal_count.
static StepArgs grid_args(const LmazeParams* p, const uint8_t* layout, const int32_t* action, int32_t* ball_xy, int32_t* goal_xy,
                          int32_t* step_count, float* reward, uint8_t* done, int32_t* goal_count, void* obs, bool u8, int64_t n,
                          int32_t auto_reset, uint64_t seed, uint64_t epoch, int64_t env_base) {
    const bool v3 = p->variant == LMAZE_VARIANT_V3;
    StepArgs a;
    a.layout = layout;
    a.action = action;
    a.ball = reinterpret_cast<int2*>(ball_xy);
    a.goal = v3 ? reinterpret_cast<const int2*>(goal_xy) : nullptr;
    a.step_count = step_count;
    a.reward = reward;
    a.done = done;
    a.goal_count = v3 ? nullptr : goal_count;
    a.obs = u8 ? nullptr : static_cast<int32_t*>(obs);
    a.obs8 = u8 ? static_cast<uint8_t*>(obs) : nullptr;
    a.n = n;
    a.grid = p->grid;
    a.step_limit = p->step_limit;
    a.reward_wall = p->reward_wall;
    a.reward_move = p->reward_move;
    a.reward_goal = p->reward_goal;
    a.envs_per_block = 0;
    a.auto_reset = auto_reset ? 1 : 0;
    a.seed = seed;
    a.epoch = epoch;
    a.env_base = env_base;
    a.epoch_in = nullptr;
    a.epoch_out = nullptr;
    a.goal_rw = v3 ? reinterpret_cast<int2*>(goal_xy) : nullptr;
    a.mask = nullptr;
    a.launch_hint = p->launch_hint;
    a.info = nullptr;
    return a;
}

// The fused reset of the *_autoreset entries and lmaze_step_u8, and the device-resident epoch words
struct FusedReset {
    int32_t auto_reset;
    uint64_t seed, epoch;
    int64_t env_base;
    const uint64_t* epoch_in;
    uint64_t* epoch_out;
};

// Every grid step / observe entry and the render of lmaze_reset.  takes: the variants the entry accepts; do_step: a step
// (action, step_count, reward and done required) or a render of the planes only (obs required, mask: just these envs); u8:
// obs is the narrow planes; fr: the entry has a fused reset.  The refusals stand in this order: params, variant, the narrow
// planes' own, LMAZE_E_NULL, LMAZE_E_ALIGN for the buffers and then the epoch words; n == 0 returns 0 after all of them.
static int grid_step(const LmazeParams* params, int takes, bool do_step, bool u8, const uint8_t* layout, const int32_t* action,
                     int32_t* ball_xy, int32_t* goal_xy, int32_t* step_count, float* reward, uint8_t* done, int32_t* goal_count,
                     void* obs, const uint8_t* mask, const FusedReset* fr, int64_t n, void* stream) {
    int rc = check_grid_params(params, n, takes, u8);
    if (rc) return rc;
    rc = check_buffers(params, u8, layout, ball_xy, goal_xy, obs, do_step ? action && step_count && reward && done : obs != nullptr);
    if (rc) return rc;
    if (fr && bad_epoch_words(fr->epoch_in, fr->epoch_out)) return LMAZE_E_ALIGN;
    const FusedReset none{0, 0, 0, 0, nullptr, nullptr};
    const FusedReset& r = fr ? *fr : none;
    StepArgs a = grid_args(params, layout, action, ball_xy, goal_xy, step_count, reward, done, goal_count, obs, u8, n, r.auto_reset,
                           r.seed, r.epoch, r.env_base);
    if (!fr) a.goal_rw = nullptr;                          // only a fused reset writes goals
    a.epoch_in = r.epoch_in;
    a.epoch_out = r.epoch_out;
    a.mask = mask;
    return (int)launch_step(params->variant, do_step, a, params->layout_mode, u8, (hipStream_t)stream);
}

namespace lmaze {
void describe_launch(LaunchInfo* info, const char* kernel, int epb, int per_cu, int chunks, bool nt, int64_t grid, int block, size_t lds) {
    snprintf(info->kernel, sizeof(info->kernel), "%s", kernel);
    info->envs_per_workgroup = epb;
    info->workgroups_per_cu = per_cu;
    info->chunks = chunks;
    info->non_temporal = nt ? 1 : 0;
    info->grid = grid;
    info->block = block;
    info->lds = (int64_t)lds;
}

int format_launch(const LaunchInfo& i, char* text, int32_t len, int32_t T) {
    if (!text || len < 1) return LMAZE_E_NULL;
    char steps[16] = "";
    if (T >= 0) snprintf(steps, sizeof(steps), " T=%d", T);
    snprintf(text, (size_t)len, "%s%s grid=%lld block=%d lds=%lld envs_per_workgroup=%d workgroups_per_cu=%d chunks=%d", i.kernel, steps,
             (long long)i.grid, i.block, (long long)i.lds, i.envs_per_workgroup, i.workgroups_per_cu, i.chunks);
    return 0;
}
}  // namespace lmaze

// The recording request of lmaze_rollout_obs / lmaze_rollout_obs_u8: refusals that need nothing else
static int check_recording(int32_t T, const void* slots, int32_t every) {
    if (every < 0 || (every == 0 && slots)) return LMAZE_E_COUNT;
    if (every > 0 && T / every > 0 && !slots) return LMAZE_E_NULL;
    if (misaligned(slots, 16)) return LMAZE_E_ALIGN;                 // u8: slot 0; the later slots start wherever N G G puts them
    return 0;
}

// What the entry path judges of a rollout's action source: the pointer it needs, that pointer's alignment (1: none; 16: the
// rows of the sampling thresholds; 4: the per-env byte tables, staged by dwords), its key mode (the action rows have none),
// whether a recording request comes with it, and whether it holds a table per env, whose rows n * G^2 must fit the int32 key
// -- and one more row the source fills whose alignment is judged (the Q-learner's td_t, floats: 4)
struct SourceChecks { const void* rows; uintptr_t align; int32_t key_mode; bool recording; bool per_env_rows; const void* filled = nullptr; };
static SourceChecks checks_of(const ActionRows& s) { return {s.actions, 1, 0, s.recording, false}; }
static SourceChecks checks_of(const PolicyTable& t) { return {t.table, 1, t.key_mode, true, false}; }
static SourceChecks checks_of(const SampleTable& t) { return {t.table, 16, t.key_mode, true, false}; }
static SourceChecks checks_of(const EnvPolicyTable& t) { return {t.table, 4, 0, true, true}; }
static SourceChecks checks_of(const EnvSampleTable& t) { return {t.table, 16, 0, true, true}; }
static SourceChecks checks_of(const EnvQTable& t) { return {t.q, 16, 0, true, true, t.td_t}; }

// Every grid rollout entry and, with info != null, its describe (then neither the recording request nor any pointer is
// judged).  slots / every: the recording request as the caller gave it.  The refusals stand in this order: the recording
// request; the params, the variant and with u8 (lmaze_step_u8's refusals) shared layouts and G >= 4 only; T; the key mode and,
// a table per env, LMAZE_E_COUNT for n * G^2 > INT32_MAX (the key is an int32 row) -- a
// bad argument is refused whether or not there is anything to do --; T == 0 or n == 0 answered before any pointer is looked
// at; LMAZE_E_NULL with the source among the pointers; LMAZE_E_ALIGN with the source's alignment among the others, and that of
// a row it fills (the Q-learner's td_t).
template <class Source>
static int grid_rollout(const LmazeParams* params, const uint8_t* layout, const Source& src, int32_t T, int32_t* ball_xy,
                        int32_t* goal_xy, int32_t* step_count, float* reward, uint8_t* done, int32_t* goal_count, void* obs, bool u8,
                        float* reward_t, uint8_t* done_t, int64_t n, int32_t auto_reset, uint64_t seed, uint64_t epoch,
                        int64_t env_base, void* slots, int32_t every, LaunchInfo* info, void* stream) {
    const SourceChecks c = checks_of(src);
    int rc = info || !c.recording ? 0 : check_recording(T, slots, every);
    if (!rc) rc = check_grid_params(params, n, TAKES_BOTH, u8);
    if (rc) return rc;
    if (T < 0) return LMAZE_E_COUNT;
    if (c.key_mode != 0 && c.key_mode != 1) return LMAZE_E_COUNT;
    if (c.key_mode == 1 && params->variant != LMAZE_VARIANT_V3) return LMAZE_E_VARIANT;   // v0 keeps no goal_xy
    if (c.per_env_rows && n * params->grid * params->grid > INT32_MAX) return LMAZE_E_COUNT;
    if (T == 0 || n == 0) return 0;                                // nothing to do, nothing read
    if (!info && (rc = check_buffers(params, u8, layout, ball_xy, goal_xy, obs, c.rows && step_count && reward && done, c.rows, c.align)) != 0)
        return rc;
    if (!info && misaligned(c.filled, 4)) return LMAZE_E_ALIGN;
    StepArgs a = grid_args(params, layout, nullptr, ball_xy, goal_xy, step_count, reward, done, goal_count, obs, u8, n, auto_reset,
                           seed, epoch, env_base);
    a.info = info;
    const RolloutRec rec{every > 0 && T / every > 0 ? slots : nullptr, every};   // the slots only where some are filled
    return (int)launch_rollout(params->variant, a, params->layout_mode, src, T, reward_t, done_t, (hipStream_t)stream, rec, u8);
}

// lmaze_describe_rollout and its closed-loop kin from the text buffer on: the line of what grid_rollout would queue, or an
// empty one.  with_obs 2: the narrow planes (the _u8 entry points).
template <class Source>
static int describe_rollout(const LmazeParams* params, const Source& src, int64_t n, int32_t T, int32_t auto_reset, int32_t with_obs,
                            int32_t obs_every, char* text_host, int32_t len) {
    if (!text_host || len < 1) return LMAZE_E_NULL;
    text_host[0] = 0;
    const bool u8 = with_obs == 2;
    LaunchInfo info{};
    // nothing is dereferenced: fabricated, aligned addresses stand for the buffers whose presence decides
    const int rc = grid_rollout(params, nullptr, src, T, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                                with_obs == 1 || u8 ? reinterpret_cast<void*>(16) : nullptr, u8, nullptr, nullptr, n, auto_reset, 0, 0, 0,
                                reinterpret_cast<void*>(32), obs_every, &info, nullptr);
    if (rc || n == 0 || T == 0) return rc;
    return format_launch(info, text_host, len);
}

// The tables of the closed-loop foveal rollouts: the pointer(s), the alignment they need (1: none), the variants the family
// takes (kTwoLevel: v5/v6 and nothing else; otherwise v1/v2/v4), a refusal of their own that stands with the counts, and
// their place in the recording struct the launcher takes (lmaze_foveal_defs.h).
struct FovealPolicyTable {
    typedef FovealRollObsPol Roll;
    static constexpr uintptr_t kAlign = 1;
    static constexpr bool kTwoLevel = false;
    const uint8_t* table;
    uint32_t epsilon;
    int refused() const { return 0; }
    bool missing() const { return !table; }
    bool unaligned() const { return false; }
    void put(Roll& ro, int32_t* actions_t, int32_t* key_t) const { ro.pol = FovealPol{table, epsilon, 0, actions_t, key_t}; }
};
struct FovealSampleTable {
    typedef FovealRollObsSmp Roll;
    static constexpr uintptr_t kAlign = 16;
    static constexpr bool kTwoLevel = false;
    const uint32_t* table;
    int refused() const { return 0; }
    bool missing() const { return !table; }
    bool unaligned() const { return misaligned(table, kAlign); }
    void put(Roll& ro, int32_t* actions_t, int32_t* key_t) const { ro.smp = FovealSmp{table, 0, actions_t, key_t}; }
};
struct FovealHierTables {
    typedef FovealRollObsHier Roll;
    static constexpr uintptr_t kAlign = 1;
    static constexpr bool kTwoLevel = true;
    const uint8_t* controller;
    const uint8_t* planner;
    uint32_t epsilon, planner_epsilon;
    int32_t controller_key;
    int32_t* goals_t;
    int32_t* goal_key_t;
    int refused() const { return controller_key != 0 && controller_key != 1 ? LMAZE_E_COUNT : 0; }
    bool missing() const { return !controller || !planner; }
    bool unaligned() const { return false; }
    void put(Roll& ro, int32_t* actions_t, int32_t* key_t) const {
        ro.hier = FovealHier{controller, planner, epsilon, planner_epsilon, controller_key, 0, actions_t, key_t, goals_t, goal_key_t};
    }
};

struct FovealHierSampleTables {
    typedef FovealRollObsHierSmp Roll;
    static constexpr uintptr_t kAlign = 16;
    static constexpr bool kTwoLevel = true;
    const uint32_t* controller;
    const uint32_t* planner;
    int32_t controller_key;
    int32_t* goals_t;
    int32_t* goal_key_t;
    int refused() const { return controller_key != 0 && controller_key != 1 ? LMAZE_E_COUNT : 0; }
    bool missing() const { return !controller || !planner; }
    bool unaligned() const { return misaligned(controller, kAlign) || misaligned(planner, kAlign); }
    void put(Roll& ro, int32_t* actions_t, int32_t* key_t) const {
        ro.hsmp = FovealHierSmp{controller, planner, controller_key, 0, actions_t, key_t, goals_t, goal_key_t};
    }
};

// lmaze_foveal_rollout_policy / lmaze_foveal_rollout_sample / lmaze_v5_rollout_policy / lmaze_v5_rollout_sample
// (lmaze_foveal_policy.hip, lmaze_foveal_sample.hip, lmaze_hier_policy.hip, lmaze_hier_sample.hip).  info != null: describe instead of launching -- then nothing past the params
// and the table's own refusal is looked at.  The refusals stand in the order include/lmaze.h documents.  obs_local_t: the
// two-level family's second recording (nullable; 16-byte aligned, refused with the recording request).
template <class Table>
static int foveal_rollout_closed(const LmazeFovealParams* params, const uint8_t* layouts, const Table& tab, int32_t T,
                                 const LmazeFovealBuffers* bufs, int64_t n, int32_t auto_reset, uint64_t seed, uint64_t epoch,
                                 int64_t env_base, float* reward_t, uint8_t* done_t, float* foveal_reward_t, uint8_t* foveal_done_t,
                                 int32_t* actions_t, int32_t* key_t, float* obs_t, float* obs_local_t, int32_t obs_every,
                                 LaunchInfo* info, void* stream) {
    int rc = check_recording(T, obs_t, obs_every);                     // 1. the recording request
    if (rc) return rc;
    if (obs_local_t && obs_every == 0) return LMAZE_E_COUNT;
    if (misaligned(obs_local_t, 16)) return LMAZE_E_ALIGN;
    rc = check_foveal_params(params);                                  // 2. the params' own refusals, the hint before the counts
    if (!rc) rc = check_foveal_hint(params);
    if (rc) return rc;
    const bool v56 = params->variant == LMAZE_VARIANT_V5 || params->variant == LMAZE_VARIANT_V6;
    if (v56 != Table::kTwoLevel) return LMAZE_E_VARIANT;               // 3. the two-level variants have a closed loop of their own
    rc = T < 0 ? LMAZE_E_COUNT : check_foveal_count(n);                // 4.
    if (!rc) rc = tab.refused();
    if (rc) return rc;
    if (T == 0 || n == 0) return 0;                                    // 5. nothing to do, nothing read
    if (!info) {                                                       // 6. the pointers, then the alignments
        if (tab.missing()) return LMAZE_E_NULL;                        // with the other pointers, before any alignment
        rc = check_foveal(params, layouts, bufs, n);
        if (rc) return rc;
        if (tab.unaligned()) return LMAZE_E_ALIGN;                     // the table's own alignment last
    }
    // the two-level step resets and plans by itself
    FovealArgs a = make_foveal_args(params, layouts, info ? nullptr : bufs, n,
                                    FovealReset{auto_reset || Table::kTwoLevel, seed, epoch, env_base, nullptr, nullptr});
    a.info = info;
    const bool rec = obs_every > 0, slots = rec && T / obs_every > 0;
    typename Table::Roll ro{FovealRollObs{FovealRoll{T, reward_t, done_t, foveal_reward_t, foveal_done_t}, slots ? obs_t : nullptr,
                                          slots ? obs_local_t : nullptr, rec ? obs_every : 1},
                            {}};
    tab.put(ro, actions_t, key_t);
    return (int)launch_foveal_rollout_closed(a, ro, rec, (hipStream_t)stream);
}

// lmaze_describe_foveal_rollout_policy / lmaze_describe_foveal_rollout_sample / lmaze_describe_v5_rollout_policy /
// lmaze_describe_v5_rollout_sample
template <class Table>
static int describe_foveal_rollout_closed(const LmazeFovealParams* params, int64_t n, int32_t T, int32_t auto_reset, int32_t obs_every,
                                          char* text_host, int32_t len, const Table& tab = Table{}) {
    if (!text_host || len < 1) return LMAZE_E_NULL;
    text_host[0] = 0;
    LaunchInfo info{};
    // nothing is dereferenced: a fabricated, aligned address stands for the slots whose presence decides
    const int rc = foveal_rollout_closed(params, nullptr, tab, T, nullptr, n, auto_reset, 0, 0, 0, nullptr, nullptr, nullptr, nullptr,
                                         nullptr, nullptr, obs_every > 0 ? reinterpret_cast<float*>(32) : nullptr, nullptr, obs_every,
                                         &info, nullptr);
    if (rc || n == 0 || T == 0) return rc;
    return format_launch(info, text_host, len, T);
}

extern "C" {

int lmaze_abi_version(void) { return LMAZE_ABI_VERSION; }

const char* lmaze_strerror(int code) {
    switch (code) {
        case 0: return "ok";
        case LMAZE_E_NULL: return "a required pointer is NULL";
        case LMAZE_E_GRID: return "grid outside [3, 64]";
        case LMAZE_E_VARIANT: return "params.variant does not match the entry point";
        case LMAZE_E_LAYOUT: return "unknown layout_mode";
        case LMAZE_E_COUNT: return "env count out of range";
        case LMAZE_E_ALIGN: return "buffer not aligned as documented";
        case LMAZE_E_EXPANSION: return "expansion ratio / channel count out of range";
        case LMAZE_E_NODEVICE: return "no usable HIP device";
        default: return code > 0 ? hipGetErrorString((hipError_t)code) : "unknown lmaze error";
    }
}

int lmaze_device_info(int device, int32_t* cu_count_host, char* name_host, int32_t name_len) {
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0 || device < 0 || device >= count) {
        (void)hipGetLastError();
        return LMAZE_E_NODEVICE;
    }
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) != hipSuccess) return LMAZE_E_NODEVICE;
    if (cu_count_host) *cu_count_host = prop.multiProcessorCount;
    if (name_host && name_len > 0) {
        strncpy(name_host, prop.gcnArchName, (size_t)name_len - 1);
        name_host[name_len - 1] = 0;
    }
    return 0;
}

int lmaze_describe_step(const LmazeParams* params, int64_t n, int32_t auto_reset, int32_t with_obs, char* text_host,
                        int32_t len) {
    int rc = check_grid_params(params, n, TAKES_BOTH, false);
    if (rc) return rc;
    if (!text_host || len < 1) return LMAZE_E_NULL;
    text_host[0] = 0;
    if (n == 0) return 0;
    const bool u8 = with_obs == 2;   // the narrow-observation step (lmaze_step_u8)
    if (u8 && (rc = check_narrow(params)) != 0) return rc;
    LaunchInfo info;
    memset(&info, 0, sizeof(info));
    // nothing is dereferenced: the launcher fills `info` where it would have queued the kernel (a fabricated, aligned
    // address stands for the planes, whose presence decides)
    StepArgs a = grid_args(params, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                           with_obs ? reinterpret_cast<void*>(16) : nullptr, u8, n, auto_reset, 0, 0, 0);
    a.info = &info;
    rc = (int)launch_step(params->variant, true, a, params->layout_mode, u8, nullptr);
    if (rc) return rc;
    return format_launch(info, text_host, len);
}

int lmaze_step_v0(const LmazeParams* params, const uint8_t* layout, const int32_t* action, int32_t* ball_xy,
                  int32_t* step_count, float* reward, uint8_t* done, int32_t* goal_count, int32_t* obs,
                  int64_t n, void* stream) {
    return grid_step(params, TAKES_V0, true, false, layout, action, ball_xy, nullptr, step_count, reward, done, goal_count, obs, nullptr,
                     nullptr, n, stream);
}

int lmaze_step_v3(const LmazeParams* params, const uint8_t* layout, const int32_t* action, int32_t* ball_xy,
                  const int32_t* goal_xy, int32_t* step_count, float* reward, uint8_t* done, int32_t* obs,
                  int64_t n, void* stream) {
    return grid_step(params, TAKES_V3, true, false, layout, action, ball_xy, const_cast<int32_t*>(goal_xy), step_count, reward, done,
                     nullptr, obs, nullptr, nullptr, n, stream);
}

int lmaze_step_v0_autoreset(const LmazeParams* params, const uint8_t* layout, const int32_t* action,
                            int32_t* ball_xy, int32_t* step_count, float* reward, uint8_t* done,
                            int32_t* goal_count, int32_t* obs, int64_t n, uint64_t seed, uint64_t epoch,
                            int64_t env_base, const uint64_t* epoch_in_dev, uint64_t* epoch_out_dev, void* stream) {
    const FusedReset fr{1, seed, epoch, env_base, epoch_in_dev, epoch_out_dev};
    return grid_step(params, TAKES_V0, true, false, layout, action, ball_xy, nullptr, step_count, reward, done, goal_count, obs, nullptr,
                     &fr, n, stream);
}

int lmaze_step_v3_autoreset(const LmazeParams* params, const uint8_t* layout, const int32_t* action,
                            int32_t* ball_xy, int32_t* goal_xy, int32_t* step_count, float* reward,
                            uint8_t* done, int32_t* obs, int64_t n, uint64_t seed, uint64_t epoch,
                            int64_t env_base, const uint64_t* epoch_in_dev, uint64_t* epoch_out_dev, void* stream) {
    const FusedReset fr{1, seed, epoch, env_base, epoch_in_dev, epoch_out_dev};
    return grid_step(params, TAKES_V3, true, false, layout, action, ball_xy, goal_xy, step_count, reward, done, nullptr, obs, nullptr,
                     &fr, n, stream);
}

int lmaze_step_u8(const LmazeParams* params, const uint8_t* layout, const int32_t* action, int32_t* ball_xy, int32_t* goal_xy,
                  int32_t* step_count, float* reward, uint8_t* done, int32_t* goal_count, uint8_t* obs8, int64_t n,
                  int32_t auto_reset, uint64_t seed, uint64_t epoch, int64_t env_base, const uint64_t* epoch_in_dev,
                  uint64_t* epoch_out_dev, void* stream) {
    const FusedReset fr{auto_reset, seed, epoch, env_base, epoch_in_dev, epoch_out_dev};
    return grid_step(params, TAKES_BOTH, true, true, layout, action, ball_xy, goal_xy, step_count, reward, done, goal_count, obs8, nullptr,
                     &fr, n, stream);
}

int lmaze_observe(const LmazeParams* params, const uint8_t* layout, const int32_t* ball_xy,
                  const int32_t* goal_xy, int32_t* obs, int64_t n, void* stream) {
    return grid_step(params, TAKES_BOTH, false, false, layout, nullptr, const_cast<int32_t*>(ball_xy), const_cast<int32_t*>(goal_xy),
                     nullptr, nullptr, nullptr, nullptr, obs, nullptr, nullptr, n, stream);
}

int lmaze_observe_u8(const LmazeParams* params, const uint8_t* layout, const int32_t* ball_xy, const int32_t* goal_xy,
                     const uint8_t* mask, uint8_t* obs8, int64_t n, void* stream) {
    return grid_step(params, TAKES_BOTH, false, true, layout, nullptr, const_cast<int32_t*>(ball_xy), const_cast<int32_t*>(goal_xy),
                     nullptr, nullptr, nullptr, nullptr, obs8, mask, nullptr, n, stream);
}

int lmaze_rollout(const LmazeParams* params, const uint8_t* layout, const int32_t* actions, int32_t T, int32_t* ball_xy,
                  int32_t* goal_xy, int32_t* step_count, float* reward, uint8_t* done, int32_t* goal_count, int32_t* obs,
                  float* reward_t, uint8_t* done_t, int64_t n, int32_t auto_reset, uint64_t seed, uint64_t epoch,
                  int64_t env_base, void* stream) {
    return grid_rollout(params, layout, ActionRows{actions, false}, T, ball_xy, goal_xy, step_count, reward, done, goal_count, obs, false,
                        reward_t, done_t, n, auto_reset, seed, epoch, env_base, nullptr, 0, nullptr, stream);
}

int lmaze_rollout_obs(const LmazeParams* params, const uint8_t* layout, const int32_t* actions, int32_t T, int32_t* ball_xy,
                      int32_t* goal_xy, int32_t* step_count, float* reward, uint8_t* done, int32_t* goal_count, int32_t* obs,
                      float* reward_t, uint8_t* done_t, int64_t n, int32_t auto_reset, uint64_t seed, uint64_t epoch,
                      int64_t env_base, int32_t* obs_t, int32_t obs_every, void* stream) {
    return grid_rollout(params, layout, ActionRows{actions, true}, T, ball_xy, goal_xy, step_count, reward, done, goal_count, obs, false,
                        reward_t, done_t, n, auto_reset, seed, epoch, env_base, obs_t, obs_every, nullptr, stream);
}

int lmaze_rollout_u8(const LmazeParams* params, const uint8_t* layout, const int32_t* actions, int32_t T, int32_t* ball_xy,
                     int32_t* goal_xy, int32_t* step_count, float* reward, uint8_t* done, int32_t* goal_count, uint8_t* obs8,
                     float* reward_t, uint8_t* done_t, int64_t n, int32_t auto_reset, uint64_t seed, uint64_t epoch,
                     int64_t env_base, void* stream) {
    return grid_rollout(params, layout, ActionRows{actions, false}, T, ball_xy, goal_xy, step_count, reward, done, goal_count, obs8, true,
                        reward_t, done_t, n, auto_reset, seed, epoch, env_base, nullptr, 0, nullptr, stream);
}

int lmaze_rollout_obs_u8(const LmazeParams* params, const uint8_t* layout, const int32_t* actions, int32_t T, int32_t* ball_xy,
                         int32_t* goal_xy, int32_t* step_count, float* reward, uint8_t* done, int32_t* goal_count, uint8_t* obs8,
                         float* reward_t, uint8_t* done_t, int64_t n, int32_t auto_reset, uint64_t seed, uint64_t epoch,
                         int64_t env_base, uint8_t* obs_t8, int32_t obs_every, void* stream) {
    return grid_rollout(params, layout, ActionRows{actions, true}, T, ball_xy, goal_xy, step_count, reward, done, goal_count, obs8, true,
                        reward_t, done_t, n, auto_reset, seed, epoch, env_base, obs_t8, obs_every, nullptr, stream);
}

int lmaze_rollout_policy(const LmazeParams* params, const uint8_t* layout, const uint8_t* policy, int32_t key_mode,
                         uint32_t epsilon_u32, int32_t T, int32_t* ball_xy, int32_t* goal_xy, int32_t* step_count, float* reward,
                         uint8_t* done, int32_t* goal_count, int32_t* obs, float* reward_t, uint8_t* done_t, int32_t* actions_t,
                         int32_t* key_t, int64_t n, int32_t auto_reset, uint64_t seed, uint64_t epoch, int64_t env_base,
                         int32_t* obs_t, int32_t obs_every, void* stream) {
    const PolicyTable tab{policy, actions_t, key_t, key_mode, epsilon_u32};
    return grid_rollout(params, layout, tab, T, ball_xy, goal_xy, step_count, reward, done, goal_count, obs, false, reward_t, done_t, n,
                        auto_reset, seed, epoch, env_base, obs_t, obs_every, nullptr, stream);
}

int lmaze_rollout_policy_u8(const LmazeParams* params, const uint8_t* layout, const uint8_t* policy, int32_t key_mode,
                            uint32_t epsilon_u32, int32_t T, int32_t* ball_xy, int32_t* goal_xy, int32_t* step_count, float* reward,
                            uint8_t* done, int32_t* goal_count, uint8_t* obs8, float* reward_t, uint8_t* done_t, int32_t* actions_t,
                            int32_t* key_t, int64_t n, int32_t auto_reset, uint64_t seed, uint64_t epoch, int64_t env_base,
                            uint8_t* obs_t8, int32_t obs_every, void* stream) {
    const PolicyTable tab{policy, actions_t, key_t, key_mode, epsilon_u32};
    return grid_rollout(params, layout, tab, T, ball_xy, goal_xy, step_count, reward, done, goal_count, obs8, true, reward_t, done_t, n,
                        auto_reset, seed, epoch, env_base, obs_t8, obs_every, nullptr, stream);
}

int lmaze_describe_rollout_policy(const LmazeParams* params, int64_t n, int32_t T, int32_t auto_reset, int32_t with_obs,
                                  int32_t obs_every, int32_t key_mode, char* text_host, int32_t len) {
    const PolicyTable tab{nullptr, nullptr, nullptr, key_mode, 0};   // obs_every and the text buffer before the params
    return obs_every < 0 ? LMAZE_E_COUNT : describe_rollout(params, tab, n, T, auto_reset, with_obs, obs_every, text_host, len);
}

int lmaze_foveal_rollout_policy(const LmazeFovealParams* params, const uint8_t* layouts, const uint8_t* policy,
                                uint32_t epsilon_u32, int32_t T, const LmazeFovealBuffers* bufs, int64_t n,
                                int32_t auto_reset, uint64_t seed, uint64_t epoch, int64_t env_base,
                                float* reward_t, uint8_t* done_t, float* foveal_reward_t, uint8_t* foveal_done_t,
                                int32_t* actions_t, int32_t* key_t, float* obs_t, int32_t obs_every, void* stream) {
    return foveal_rollout_closed(params, layouts, FovealPolicyTable{policy, epsilon_u32}, T, bufs, n, auto_reset, seed, epoch, env_base,
                                 reward_t, done_t, foveal_reward_t, foveal_done_t, actions_t, key_t, obs_t, nullptr, obs_every, nullptr,
                                 stream);
}

int lmaze_describe_foveal_rollout_policy(const LmazeFovealParams* params, int64_t n, int32_t T, int32_t auto_reset,
                                         int32_t obs_every, char* text_host, int32_t len) {
    return describe_foveal_rollout_closed<FovealPolicyTable>(params, n, T, auto_reset, obs_every, text_host, len);
}

int lmaze_v5_rollout_policy(const LmazeFovealParams* params, const uint8_t* layouts, const uint8_t* controller, int32_t controller_key,
                            uint32_t epsilon_u32, const uint8_t* planner, uint32_t planner_epsilon_u32, int32_t T,
                            const LmazeFovealBuffers* bufs, int64_t n, uint64_t seed, uint64_t epoch, int64_t env_base, float* reward_t,
                            uint8_t* done_t, float* foveal_reward_t, uint8_t* foveal_done_t, int32_t* actions_t, int32_t* key_t,
                            int32_t* goals_t, int32_t* goal_key_t, float* obs_t, float* obs_local_t, int32_t obs_every, void* stream) {
    const FovealHierTables tab{controller, planner, epsilon_u32, planner_epsilon_u32, controller_key, goals_t, goal_key_t};
    return foveal_rollout_closed(params, layouts, tab, T, bufs, n, 1, seed, epoch, env_base, reward_t, done_t, foveal_reward_t,
                                 foveal_done_t, actions_t, key_t, obs_t, obs_local_t, obs_every, nullptr, stream);
}

int lmaze_describe_v5_rollout_policy(const LmazeFovealParams* params, int64_t n, int32_t T, int32_t controller_key, int32_t obs_every,
                                     char* text_host, int32_t len) {
    const FovealHierTables tab{nullptr, nullptr, 0, 0, controller_key, nullptr, nullptr};
    return describe_foveal_rollout_closed(params, n, T, 1, obs_every, text_host, len, tab);
}

int lmaze_v5_rollout_sample(const LmazeFovealParams* params, const uint8_t* layouts, const uint32_t* controller_thresholds,
                            int32_t controller_key, const uint32_t* planner_thresholds, int32_t T, const LmazeFovealBuffers* bufs,
                            int64_t n, uint64_t seed, uint64_t epoch, int64_t env_base, float* reward_t, uint8_t* done_t,
                            float* foveal_reward_t, uint8_t* foveal_done_t, int32_t* actions_t, int32_t* key_t, int32_t* goals_t,
                            int32_t* goal_key_t, float* obs_t, float* obs_local_t, int32_t obs_every, void* stream) {
    const FovealHierSampleTables tab{controller_thresholds, planner_thresholds, controller_key, goals_t, goal_key_t};
    return foveal_rollout_closed(params, layouts, tab, T, bufs, n, 1, seed, epoch, env_base, reward_t, done_t, foveal_reward_t,
                                 foveal_done_t, actions_t, key_t, obs_t, obs_local_t, obs_every, nullptr, stream);
}

int lmaze_describe_v5_rollout_sample(const LmazeFovealParams* params, int64_t n, int32_t T, int32_t controller_key, int32_t obs_every,
                                     char* text_host, int32_t len) {
    const FovealHierSampleTables tab{nullptr, nullptr, controller_key, nullptr, nullptr};
    return describe_foveal_rollout_closed(params, n, T, 1, obs_every, text_host, len, tab);
}

int lmaze_foveal_rollout_sample(const LmazeFovealParams* params, const uint8_t* layouts, const uint32_t* thresholds, int32_t T,
                                const LmazeFovealBuffers* bufs, int64_t n, int32_t auto_reset, uint64_t seed, uint64_t epoch,
                                int64_t env_base, float* reward_t, uint8_t* done_t, float* foveal_reward_t, uint8_t* foveal_done_t,
                                int32_t* actions_t, int32_t* key_t, float* obs_t, int32_t obs_every, void* stream) {
    return foveal_rollout_closed(params, layouts, FovealSampleTable{thresholds}, T, bufs, n, auto_reset, seed, epoch, env_base,
                                 reward_t, done_t, foveal_reward_t, foveal_done_t, actions_t, key_t, obs_t, nullptr, obs_every, nullptr,
                                 stream);
}

int lmaze_describe_foveal_rollout_sample(const LmazeFovealParams* params, int64_t n, int32_t T, int32_t auto_reset,
                                         int32_t obs_every, char* text_host, int32_t len) {
    return describe_foveal_rollout_closed<FovealSampleTable>(params, n, T, auto_reset, obs_every, text_host, len);
}

int lmaze_rollout_sample(const LmazeParams* params, const uint8_t* layout, const uint32_t* thresholds, int32_t key_mode, int32_t T,
                         int32_t* ball_xy, int32_t* goal_xy, int32_t* step_count, float* reward, uint8_t* done, int32_t* goal_count,
                         int32_t* obs, float* reward_t, uint8_t* done_t, int32_t* actions_t, int32_t* key_t, int64_t n,
                         int32_t auto_reset, uint64_t seed, uint64_t epoch, int64_t env_base, int32_t* obs_t, int32_t obs_every,
                         void* stream) {
    const SampleTable tab{reinterpret_cast<const sample_row_t*>(thresholds), actions_t, key_t, key_mode, 0};
    return grid_rollout(params, layout, tab, T, ball_xy, goal_xy, step_count, reward, done, goal_count, obs, false, reward_t, done_t, n,
                        auto_reset, seed, epoch, env_base, obs_t, obs_every, nullptr, stream);
}

int lmaze_rollout_sample_u8(const LmazeParams* params, const uint8_t* layout, const uint32_t* thresholds, int32_t key_mode, int32_t T,
                            int32_t* ball_xy, int32_t* goal_xy, int32_t* step_count, float* reward, uint8_t* done,
                            int32_t* goal_count, uint8_t* obs8, float* reward_t, uint8_t* done_t, int32_t* actions_t, int32_t* key_t,
                            int64_t n, int32_t auto_reset, uint64_t seed, uint64_t epoch, int64_t env_base, uint8_t* obs_t8,
                            int32_t obs_every, void* stream) {
    const SampleTable tab{reinterpret_cast<const sample_row_t*>(thresholds), actions_t, key_t, key_mode, 0};
    return grid_rollout(params, layout, tab, T, ball_xy, goal_xy, step_count, reward, done, goal_count, obs8, true, reward_t, done_t, n,
                        auto_reset, seed, epoch, env_base, obs_t8, obs_every, nullptr, stream);
}

int lmaze_describe_rollout_sample(const LmazeParams* params, int64_t n, int32_t T, int32_t auto_reset, int32_t with_obs,
                                  int32_t obs_every, int32_t key_mode, char* text_host, int32_t len) {
    const SampleTable tab{nullptr, nullptr, nullptr, key_mode, 0};
    return obs_every < 0 ? LMAZE_E_COUNT : describe_rollout(params, tab, n, T, auto_reset, with_obs, obs_every, text_host, len);
}

int lmaze_env_rollout_policy(const LmazeParams* params, const uint8_t* layout, const uint8_t* policy, uint32_t epsilon_u32,
                             int32_t T, int32_t* ball_xy, int32_t* goal_xy, int32_t* step_count, float* reward, uint8_t* done,
                             int32_t* goal_count, int32_t* obs, float* reward_t, uint8_t* done_t, int32_t* actions_t, int32_t* key_t,
                             int64_t n, int32_t auto_reset, uint64_t seed, uint64_t epoch, int64_t env_base, int32_t* obs_t,
                             int32_t obs_every, void* stream) {
    const EnvPolicyTable tab{policy, actions_t, key_t, epsilon_u32};
    return grid_rollout(params, layout, tab, T, ball_xy, goal_xy, step_count, reward, done, goal_count, obs, false, reward_t, done_t, n,
                        auto_reset, seed, epoch, env_base, obs_t, obs_every, nullptr, stream);
}

int lmaze_env_rollout_sample(const LmazeParams* params, const uint8_t* layout, const uint32_t* thresholds, int32_t T,
                             int32_t* ball_xy, int32_t* goal_xy, int32_t* step_count, float* reward, uint8_t* done,
                             int32_t* goal_count, int32_t* obs, float* reward_t, uint8_t* done_t, int32_t* actions_t, int32_t* key_t,
                             int64_t n, int32_t auto_reset, uint64_t seed, uint64_t epoch, int64_t env_base, int32_t* obs_t,
                             int32_t obs_every, void* stream) {
    const EnvSampleTable tab{reinterpret_cast<const sample_row_t*>(thresholds), actions_t, key_t};
    return grid_rollout(params, layout, tab, T, ball_xy, goal_xy, step_count, reward, done, goal_count, obs, false, reward_t, done_t, n,
                        auto_reset, seed, epoch, env_base, obs_t, obs_every, nullptr, stream);
}

int lmaze_describe_env_rollout(const LmazeParams* params, int64_t n, int32_t T, int32_t auto_reset, int32_t with_obs,
                               int32_t obs_every, int32_t form, char* text_host, int32_t len) {
    if (obs_every < 0 || with_obs == 2 || (form != 0 && form != 1)) return LMAZE_E_COUNT;   // no narrow planes; 0 policy, 1 sample
    if (form == 0) return describe_rollout(params, EnvPolicyTable{nullptr, nullptr, nullptr, 0}, n, T, auto_reset, with_obs, obs_every, text_host, len);
    return describe_rollout(params, EnvSampleTable{nullptr, nullptr, nullptr}, n, T, auto_reset, with_obs, obs_every, text_host, len);
}

int lmaze_env_rollout_qlearn(const LmazeParams* params, const uint8_t* layout, float* q, float alpha, float gamma,
                             uint32_t epsilon_u32, int32_t T, int32_t* ball_xy, int32_t* goal_xy, int32_t* step_count, float* reward,
                             uint8_t* done, int32_t* goal_count, int32_t* obs, float* reward_t, uint8_t* done_t, int32_t* actions_t,
                             int32_t* key_t, float* td_t, int64_t n, int32_t auto_reset, uint64_t seed, uint64_t epoch,
                             int64_t env_base, int32_t* obs_t, int32_t obs_every, void* stream) {
    const EnvQTable tab{reinterpret_cast<q_row_t*>(q), alpha, gamma, epsilon_u32, actions_t, key_t, td_t};
    return grid_rollout(params, layout, tab, T, ball_xy, goal_xy, step_count, reward, done, goal_count, obs, false, reward_t, done_t, n,
                        auto_reset, seed, epoch, env_base, obs_t, obs_every, nullptr, stream);
}

int lmaze_describe_env_rollout_qlearn(const LmazeParams* params, int64_t n, int32_t T, int32_t auto_reset, int32_t with_obs,
                                      int32_t obs_every, char* text_host, int32_t len) {
    if (obs_every < 0 || with_obs == 2) return LMAZE_E_COUNT;      // no narrow planes
    return describe_rollout(params, EnvQTable{nullptr, 0.0f, 0.0f, 0, nullptr, nullptr, nullptr}, n, T, auto_reset, with_obs, obs_every,
                            text_host, len);
}

int lmaze_returns(const float* reward_t, const uint8_t* done_t, const float* tail, float gamma, float* returns_t, int32_t T,
                  int64_t n, void* stream) {
    if (!reward_t || !done_t || !returns_t) return LMAZE_E_NULL;
    if (T < 0 || n < 0 || n > LMAZE_MAX_ENVS) return LMAZE_E_COUNT;
    return (int)launch_returns(reward_t, done_t, tail, gamma, returns_t, T, n, (hipStream_t)stream);
}

static int advantages(const AdvantageArgs& a, bool required, int64_t keys, void* stream) {
    if (!required) return LMAZE_E_NULL;
    if (a.T < 0 || a.n < 0 || a.n > LMAZE_MAX_ENVS || keys < 1) return LMAZE_E_COUNT;
    return (int)launch_advantages(a, (hipStream_t)stream);
}

int lmaze_advantages(const float* reward_t, const uint8_t* done_t, const float* value_t, const float* tail, float gamma, float lambda,
                     float* adv_t, float* target_t, int32_t T, int64_t n, void* stream) {
    const AdvantageArgs a{reward_t, done_t, value_t, tail, nullptr, nullptr, nullptr, 0, gamma, gamma * lambda, adv_t, target_t, T, n};
    return advantages(a, reward_t && done_t && value_t && adv_t, 1, stream);
}

int lmaze_advantages_table(const float* reward_t, const uint8_t* done_t, const int32_t* key_t, const int32_t* key_tail,
                           const float* values, int64_t keys, float gamma, float lambda, float* adv_t, float* target_t, int32_t T,
                           int64_t n, void* stream) {
    // an int32 key is compared unsigned: a table beyond 2^31 entries has no key that could reach past it
    const uint32_t ku = keys > ((int64_t)1 << 31) ? (uint32_t)1 << 31 : (uint32_t)(keys < 0 ? 0 : keys);
    const AdvantageArgs a{reward_t, done_t, nullptr, nullptr, key_t, key_tail, values, ku, gamma, gamma * lambda, adv_t, target_t, T, n};
    return advantages(a, reward_t && done_t && key_t && values && adv_t, keys, stream);
}

// One table of the off-policy entries, in exactly one of lmaze_evaluate's three forms; *law is filled when it is.
static bool action_law(const uint8_t* policy, const float* q, uint32_t epsilon_u32, const uint32_t* thresholds, ActionLaw* law) {
    if ((policy != nullptr) + (q != nullptr) + (thresholds != nullptr) != 1) return false;
    law->policy = policy;
    law->rows = q ? reinterpret_cast<const uint4*>(q) : reinterpret_cast<const uint4*>(thresholds);
    law->form = policy ? LMAZE_LAW_POLICY : (q ? LMAZE_LAW_Q : LMAZE_LAW_THRESHOLDS);
    law->epsilon = epsilon_u32;
    return true;
}

// an int32 key is compared unsigned: a table beyond 2^31 entries has no key that could reach past it (keys >= 1)
static uint32_t key_count(int64_t keys) { return keys > ((int64_t)1 << 31) ? (uint32_t)1 << 31 : (uint32_t)keys; }

int lmaze_action_probs(const int32_t* key_t, const int32_t* actions_t, int64_t m, const uint8_t* policy, const float* q,
                       uint32_t epsilon_u32, const uint32_t* thresholds, int64_t keys, float* prob_t, void* stream) {
    if (!key_t || !actions_t || !prob_t) return LMAZE_E_NULL;
    ActionProbsArgs a{};
    if (!action_law(policy, q, epsilon_u32, thresholds, &a.law)) return LMAZE_E_NULL;
    if (m < 0 || keys < 1) return LMAZE_E_COUNT;
    if (misaligned(a.law.rows, 16) || misaligned(key_t, 4) || misaligned(actions_t, 4) || misaligned(prob_t, 4)) return LMAZE_E_ALIGN;
    if (m == 0) return 0;
    a.key_t = key_t;
    a.actions_t = actions_t;
    a.keys = key_count(keys);
    a.prob_t = prob_t;
    a.m = m;
    return (int)launch_action_probs(a, (hipStream_t)stream);
}

// what lmaze_vtrace and lmaze_vtrace_table judge alike, behind their own pointers and tables
static int vtrace(const VtraceArgs& a, int64_t keys, void* stream) {
    if (a.T < 0 || a.n < 0 || a.n > LMAZE_MAX_ENVS || keys < 1) return LMAZE_E_COUNT;
    if (misaligned(a.behaviour.rows, 16) || misaligned(a.target.rows, 16) || misaligned(a.reward_t, 4) || misaligned(a.value_t, 4) ||
        misaligned(a.tail, 4) || misaligned(a.rho_t, 4) || misaligned(a.key_t, 4) || misaligned(a.actions_t, 4) ||
        misaligned(a.key_tail, 4) || misaligned(a.values, 4) || misaligned(a.vs_t, 4) || misaligned(a.pg_t, 4) ||
        misaligned(a.rho_out_t, 4))
        return LMAZE_E_ALIGN;
    return (int)launch_vtrace(a, (hipStream_t)stream);
}

int lmaze_vtrace(const float* reward_t, const uint8_t* done_t, const float* value_t, const float* tail, const float* rho_t,
                 float gamma, float lambda, float rho_bar, float c_bar, float* vs_t, float* pg_adv_t, int32_t T, int64_t n, void* stream) {
    if (!reward_t || !done_t || !value_t || (!vs_t && !pg_adv_t)) return LMAZE_E_NULL;
    VtraceArgs a{};
    a.reward_t = reward_t;
    a.done_t = done_t;
    a.value_t = value_t;
    a.tail = tail;
    a.rho_t = rho_t;
    a.gamma = gamma;
    a.lambda = lambda;
    a.rho_bar = rho_bar;
    a.c_bar = c_bar;
    a.vs_t = vs_t;
    a.pg_t = pg_adv_t;
    a.T = T;
    a.n = n;
    return vtrace(a, 1, stream);
}

int lmaze_vtrace_table(const float* reward_t, const uint8_t* done_t, const int32_t* key_t, const int32_t* actions_t,
                       const int32_t* key_tail, const float* values, int64_t keys, const uint8_t* b_policy, const float* b_q,
                       uint32_t b_epsilon_u32, const uint32_t* b_thresholds, const uint8_t* t_policy, const float* t_q,
                       uint32_t t_epsilon_u32, const uint32_t* t_thresholds, float gamma, float lambda, float rho_bar, float c_bar,
                       float* vs_t, float* pg_adv_t, float* rho_out_t, int32_t T, int64_t n, void* stream) {
    if (!reward_t || !done_t || !key_t || !actions_t || !values || (!vs_t && !pg_adv_t)) return LMAZE_E_NULL;
    VtraceArgs a{};
    if (!action_law(b_policy, b_q, b_epsilon_u32, b_thresholds, &a.behaviour)) return LMAZE_E_NULL;
    if (!action_law(t_policy, t_q, t_epsilon_u32, t_thresholds, &a.target)) return LMAZE_E_NULL;
    a.reward_t = reward_t;
    a.done_t = done_t;
    a.key_t = key_t;
    a.actions_t = actions_t;
    a.key_tail = key_tail;
    a.values = values;
    a.keys = keys < 1 ? 0 : key_count(keys);
    a.gamma = gamma;
    a.lambda = lambda;
    a.rho_bar = rho_bar;
    a.c_bar = c_bar;
    a.vs_t = vs_t;
    a.pg_t = pg_adv_t;
    a.rho_out_t = rho_out_t;
    a.T = T;
    a.n = n;
    return vtrace(a, keys, stream);
}

static int check_table_stats(const void* key_t, const void* actions_t, const void* weight_t, int64_t m, int64_t keys, int32_t actions,
                             const void* count, const void* total) {
    if (!key_t || !count) return LMAZE_E_NULL;
    if ((weight_t != nullptr) != (total != nullptr)) return LMAZE_E_NULL;
    if (m < 0 || keys < 1 || actions < 1 || actions > 255 || keys > ((int64_t)1 << 28) || keys * actions > ((int64_t)1 << 28))
        return LMAZE_E_COUNT;
    if (!actions_t && actions != 1) return LMAZE_E_COUNT;
    return 0;
}

int lmaze_table_stats(const int32_t* key_t, const int32_t* actions_t, const float* weight_t, int64_t m, int64_t keys, int32_t actions,
                      int64_t* count, int64_t* total_q24, void* stream) {
    const int rc = check_table_stats(key_t, actions_t, weight_t, m, keys, actions, count, total_q24);
    if (rc || m == 0) return rc;
    if (misaligned(key_t, 4) || misaligned(actions_t, 4) || misaligned(weight_t, 4) || misaligned(count, 8) || misaligned(total_q24, 8))
        return LMAZE_E_ALIGN;
    const TableStatsArgs a{key_t, actions_t, weight_t, m, (uint32_t)keys, (uint32_t)actions,
                           reinterpret_cast<unsigned long long*>(count), reinterpret_cast<unsigned long long*>(total_q24)};
    return (int)launch_table_stats(a, (hipStream_t)stream);
}

int lmaze_describe_table_stats(int64_t m, int64_t keys, int32_t actions, char* text_host, int32_t len) {
    if (!text_host || len < 1) return LMAZE_E_NULL;
    text_host[0] = 0;
    // nothing is dereferenced: fabricated addresses stand for the rows, whose presence decides nothing the line reports
    const int rc = check_table_stats(text_host, actions == 1 ? nullptr : text_host, nullptr, m, keys, actions, text_host, nullptr);
    if (rc || m == 0) return rc;
    const TableStatsPlan p = plan_table_stats(m, keys, actions);
    snprintf(text_host, (size_t)len, "table_stats_kernel<%s> grid=%lld block=%d lds=%lld bins=%lld", p.lds ? "lds" : "global",
             (long long)p.grid, LMAZE_BLOCK, (long long)p.lds_bytes, (long long)p.bins);
    return 0;
}

// What lmaze_solve and lmaze_describe_solve judge of the params, in the header's order (the variant before the layout mode)
static int check_solve_params(const LmazeParams* p) {
    if (p->grid < 3 || p->grid > LMAZE_MAX_GRID) return LMAZE_E_GRID;
    if (p->variant != LMAZE_VARIANT_V0 && p->variant != LMAZE_VARIANT_V3) return LMAZE_E_VARIANT;
    if (p->layout_mode != LMAZE_LAYOUT_SHARED && p->layout_mode != LMAZE_LAYOUT_PER_ENV) return LMAZE_E_LAYOUT;
    return 0;
}

// The head lmaze_solve, lmaze_score, lmaze_evaluate and lmaze_occupancy judge alike, before anything of their own: params and layouts, the
// params' values, v3's goal
static int check_problems_head(const LmazeParams* params, const uint8_t* layouts, const int32_t* goal_xy) {
    if (!params || !layouts) return LMAZE_E_NULL;
    const int rc = check_solve_params(params);
    if (rc) return rc;
    if (params->variant == LMAZE_VARIANT_V3 && !goal_xy) return LMAZE_E_NULL;
    return 0;
}

// ... and the tail, behind their own pointers: the counts (the entry's own with the problems' range), the alignments (the
// entry's own with the goal's).  The caller returns the code, or 0 when problems == 0: nothing to do
static int check_problems_tail(const LmazeParams* params, const int32_t* goal_xy, int64_t problems, bool own_counts_ok,
                               bool own_aligned) {
    if (problems < 0 || problems > LMAZE_MAX_ENVS || !own_counts_ok) return LMAZE_E_COUNT;
    if (!own_aligned || (params->variant == LMAZE_VARIANT_V3 && misaligned(goal_xy, 8))) return LMAZE_E_ALIGN;
    return 0;
}

int lmaze_solve(const LmazeParams* params, const uint8_t* layouts, const int32_t* goal_xy, int64_t problems, float gamma,
                int32_t sweeps, const float* v_init, float* q, float* v, uint8_t* policy, int32_t* sweeps_run, float* delta,
                void* stream) {
    int rc = check_problems_head(params, layouts, goal_xy);
    if (rc) return rc;
    if (!q && !v && !policy) return LMAZE_E_NULL;
    rc = check_problems_tail(params, goal_xy, problems, sweeps >= 1,
                             !(misaligned(q, 16) || misaligned(v_init, 4) || misaligned(v, 4) || misaligned(sweeps_run, 4) ||
                               misaligned(delta, 4)));
    if (rc || problems == 0) return rc;
    SolveArgs a = problem_args<SolveArgs>(params, layouts, goal_xy, problems);
    a.v_init = v_init;
    a.q = reinterpret_cast<float4*>(q);
    a.v = v;
    a.policy = policy;
    a.sweeps_run = sweeps_run;
    a.delta = delta;
    a.sweeps = sweeps;
    a.gamma = gamma;
    return (int)launch_solve(params->variant, a, (hipStream_t)stream);
}

int lmaze_score(const LmazeParams* params, const uint8_t* layouts, const int32_t* goal_xy, int64_t problems, const uint8_t* policy,
                const float* q, int32_t* optimal, int32_t* steps, int32_t* summary, void* stream) {
    int rc = check_problems_head(params, layouts, goal_xy);
    if (rc) return rc;
    if (!optimal && !steps && !summary) return LMAZE_E_NULL;
    if (policy && q) return LMAZE_E_NULL;
    if (steps && !policy && !q) return LMAZE_E_NULL;
    rc = check_problems_tail(params, goal_xy, problems, true,
                             !(misaligned(q, 16) || misaligned(policy, 4) || misaligned(optimal, 4) || misaligned(steps, 4) ||
                               misaligned(summary, 4)));
    if (rc || problems == 0) return rc;
    ScoreArgs a = problem_args<ScoreArgs>(params, layouts, goal_xy, problems);
    a.policy = policy;
    a.q = reinterpret_cast<const float4*>(q);
    a.optimal = optimal;
    a.steps = steps;
    a.summary = summary;
    return (int)launch_score(params->variant, a, (hipStream_t)stream);
}

int lmaze_evaluate(const LmazeParams* params, const uint8_t* layouts, const int32_t* goal_xy, int64_t problems, const uint8_t* policy,
                   const float* q, uint32_t epsilon_u32, const uint32_t* thresholds, float gamma, int32_t sweeps, float tol,
                   const float* v_init, float* q_out, float* v_out, int32_t* sweeps_run, float* delta, void* stream) {
    int rc = check_problems_head(params, layouts, goal_xy);
    if (rc) return rc;
    if (!q_out && !v_out) return LMAZE_E_NULL;
    if ((policy ? 1 : 0) + (q ? 1 : 0) + (thresholds ? 1 : 0) != 1) return LMAZE_E_NULL;
    rc = check_problems_tail(params, goal_xy, problems, sweeps >= 1,
                             !(misaligned(thresholds, 16) || misaligned(q, 16) || misaligned(q_out, 16) || misaligned(v_init, 4) ||
                               misaligned(v_out, 4) || misaligned(sweeps_run, 4) || misaligned(delta, 4)));
    if (rc || problems == 0) return rc;
    EvaluateArgs a = problem_args<EvaluateArgs>(params, layouts, goal_xy, problems);
    a.policy = policy;
    a.q = reinterpret_cast<const float4*>(q);
    a.thresholds = reinterpret_cast<const uint4*>(thresholds);
    a.v_init = v_init;
    a.q_out = reinterpret_cast<float4*>(q_out);
    a.v_out = v_out;
    a.sweeps_run = sweeps_run;
    a.delta = delta;
    a.sweeps = sweeps;
    a.epsilon = epsilon_u32;
    a.gamma = gamma;
    a.tol = tol;
    return (int)launch_evaluate(params->variant, a, (hipStream_t)stream);
}

int lmaze_occupancy(const LmazeParams* params, const uint8_t* layouts, const int32_t* goal_xy, int64_t problems, const uint8_t* policy,
                    const float* q, uint32_t epsilon_u32, const uint32_t* thresholds, const float* start, float gamma, int32_t sweeps,
                    float tol, const float* d_init, float* d_out, float* dsa_out, int32_t* sweeps_run, float* delta, void* stream) {
    int rc = check_problems_head(params, layouts, goal_xy);
    if (rc) return rc;
    if (!d_out && !dsa_out) return LMAZE_E_NULL;
    if ((policy ? 1 : 0) + (q ? 1 : 0) + (thresholds ? 1 : 0) != 1) return LMAZE_E_NULL;
    if (!start) return LMAZE_E_NULL;
    rc = check_problems_tail(params, goal_xy, problems, sweeps >= 1,
                             !(misaligned(thresholds, 16) || misaligned(q, 16) || misaligned(dsa_out, 16) || misaligned(start, 4) ||
                               misaligned(d_init, 4) || misaligned(d_out, 4) || misaligned(sweeps_run, 4) || misaligned(delta, 4)));
    if (rc || problems == 0) return rc;
    OccupancyArgs a = problem_args<OccupancyArgs>(params, layouts, goal_xy, problems);
    a.policy = policy;
    a.q = reinterpret_cast<const float4*>(q);
    a.thresholds = reinterpret_cast<const uint4*>(thresholds);
    a.start = start;
    a.d_init = d_init;
    a.d_out = d_out;
    a.dsa_out = reinterpret_cast<float4*>(dsa_out);
    a.sweeps_run = sweeps_run;
    a.delta = delta;
    a.sweeps = sweeps;
    a.epsilon = epsilon_u32;
    a.gamma = gamma;
    a.tol = tol;
    return (int)launch_occupancy(params->variant, a, (hipStream_t)stream);
}

// what the four lmaze_describe_* judge and print: `kernel` names the family's kernel
static int describe_problems(const LmazeParams* params, int64_t problems, char* text_host, int32_t len, const char* kernel) {
    if (!params || !text_host || len < 1) return LMAZE_E_NULL;
    text_host[0] = 0;
    const int rc = check_solve_params(params);
    if (rc) return rc;
    if (problems < 0 || problems > LMAZE_MAX_ENVS) return LMAZE_E_COUNT;
    if (problems == 0) return 0;
    return describe_problems_plan(kernel, params->variant, plan_solve(params->grid, problems), text_host, len);
}

int lmaze_describe_solve(const LmazeParams* params, int64_t problems, char* text_host, int32_t len) {
    return describe_problems(params, problems, text_host, len, "solve_kernel");
}

int lmaze_describe_score(const LmazeParams* params, int64_t problems, char* text_host, int32_t len) {
    return describe_problems(params, problems, text_host, len, "score_kernel");
}

int lmaze_describe_evaluate(const LmazeParams* params, int64_t problems, char* text_host, int32_t len) {
    return describe_problems(params, problems, text_host, len, "evaluate_kernel");
}

int lmaze_describe_occupancy(const LmazeParams* params, int64_t problems, char* text_host, int32_t len) {
    return describe_problems(params, problems, text_host, len, "occupancy_kernel");
}

// What lmaze_generate and lmaze_describe_generate judge of the grid side and of the counts, in the header's order
static int check_generate_counts(int32_t grid, int64_t mazes, int64_t maze_base) {
    if (grid < 5 || grid > LMAZE_MAX_GRID) return LMAZE_E_GRID;
    if (mazes < 0 || mazes > LMAZE_MAX_ENVS || maze_base < 0 || maze_base > INT64_MAX - mazes) return LMAZE_E_COUNT;
    return 0;
}

int lmaze_generate(int32_t grid, int64_t mazes, uint64_t seed, int64_t maze_base, uint32_t loops_u32, uint8_t* layouts,
                   int32_t* goal_xy, void* stream) {
    if (!layouts) return LMAZE_E_NULL;
    const int rc = check_generate_counts(grid, mazes, maze_base);
    if (rc) return rc;
    if (misaligned(layouts, 16) || misaligned(goal_xy, 8)) return LMAZE_E_ALIGN;
    if (mazes == 0) return 0;
    const GenerateArgs a{layouts, reinterpret_cast<int2*>(goal_xy), mazes, maze_base, seed, loops_u32, grid};
    return (int)launch_generate(a, (hipStream_t)stream);
}

int lmaze_describe_generate(int32_t grid, int64_t mazes, char* text_host, int32_t len) {
    if (!text_host || len < 1) return LMAZE_E_NULL;
    text_host[0] = 0;
    const int rc = check_generate_counts(grid, mazes, 0);
    if (rc || mazes == 0) return rc;
    return describe_generate(plan_generate(grid, mazes), text_host, len);
}

int lmaze_describe_rollout(const LmazeParams* params, int64_t n, int32_t T, int32_t auto_reset, int32_t with_obs, int32_t obs_every,
                           char* text_host, int32_t len) {
    // this describe's own order: the params, the variant and T before the text buffer, and the narrow planes' refusals
    // (grid_rollout's) only when there is something to do
    int rc = check_grid_params(params, n, TAKES_BOTH, false);
    if (!rc && T < 0) rc = LMAZE_E_COUNT;
    if (rc || !text_host || len < 1) return rc ? rc : LMAZE_E_NULL;
    text_host[0] = 0;
    if (n == 0 || T == 0) return 0;
    return describe_rollout(params, ActionRows{nullptr, obs_every >= 0}, n, T, auto_reset, with_obs, obs_every, text_host, len);
}

int lmaze_reset(const LmazeParams* params, const uint8_t* layout, const uint8_t* mask, uint64_t seed,
                uint64_t epoch, int64_t env_base, int32_t* ball_xy, int32_t* goal_xy, int32_t* step_count, float* reward,
                uint8_t* done, int32_t* obs, int64_t n, void* stream) {
    int rc = check_grid_params(params, n, TAKES_BOTH, false);
    if (rc) return rc;
    rc = check_buffers(params, false, layout, ball_xy, goal_xy, obs, step_count && reward && done);
    if (rc) return rc;
    ResetArgs r;
    r.layout = layout;
    r.mask = mask;
    r.ball = reinterpret_cast<int2*>(ball_xy);
    r.goal = reinterpret_cast<int2*>(goal_xy);
    r.step_count = step_count;
    r.reward = reward;
    r.done = done;
    r.n = n;
    r.seed = seed;
    r.epoch = epoch;
    r.env_base = env_base;
    r.grid = params->grid;
    hipError_t e = launch_reset(params->variant, r, params->layout_mode, (hipStream_t)stream);
    if (e != hipSuccess || !obs) return (int)e;
    // only the envs that were reset are re-rendered
    return grid_step(params, TAKES_BOTH, false, false, layout, nullptr, ball_xy, goal_xy, nullptr, nullptr, nullptr, nullptr, obs, mask,
                     nullptr, n, stream);
}

// What lmaze_reset_start and its describe refuse of the row mode: LMAZE_E_COUNT outside {0, 1, 2}, then LMAZE_E_VARIANT for
// what v0 has no goal for
static int check_row_mode(const LmazeParams* p, int32_t row_mode, int32_t keep_goal) {
    if (row_mode < 0 || row_mode > 2) return LMAZE_E_COUNT;
    if (p->variant == LMAZE_VARIANT_V0 && (row_mode == 2 || keep_goal)) return LMAZE_E_VARIANT;
    return 0;
}

int lmaze_reset_start(const LmazeParams* params, const uint8_t* layout, const uint8_t* mask, const uint32_t* thresholds,
                      int32_t row_mode, int32_t keep_goal, uint64_t seed, uint64_t epoch, int64_t env_base, int32_t* ball_xy,
                      int32_t* goal_xy, int32_t* step_count, float* reward, uint8_t* done, int32_t* obs, int64_t n, void* stream) {
    int rc = check_grid_params(params, n, TAKES_BOTH, false);
    if (rc) return rc;
    rc = check_buffers(params, false, layout, ball_xy, goal_xy, obs, step_count && reward && done);
    if (rc) return rc;
    rc = check_row_mode(params, row_mode, keep_goal);
    if (rc) return rc;
    if (!thresholds) return LMAZE_E_NULL;
    if (misaligned(thresholds, 4)) return LMAZE_E_ALIGN;
    if (n == 0) return 0;
    ResetStartArgs a;
    a.r.layout = layout;
    a.r.mask = mask;
    a.r.ball = reinterpret_cast<int2*>(ball_xy);
    a.r.goal = reinterpret_cast<int2*>(goal_xy);
    a.r.step_count = step_count;
    a.r.reward = reward;
    a.r.done = done;
    a.r.n = n;
    a.r.seed = seed;
    a.r.epoch = epoch;
    a.r.env_base = env_base;
    a.r.grid = params->grid;
    a.thresholds = thresholds;
    a.row_mode = row_mode;
    a.keep_goal = keep_goal ? 1 : 0;
    a.per_env = a.top = 0;                                 // the launcher's
    hipError_t e = launch_reset_start(params->variant, a, params->layout_mode, (hipStream_t)stream, nullptr);
    if (e != hipSuccess || !obs) return (int)e;
    // only the envs that were reset are re-rendered, as lmaze_reset's
    return grid_step(params, TAKES_BOTH, false, false, layout, nullptr, ball_xy, goal_xy, nullptr, nullptr, nullptr, nullptr, obs, mask,
                     nullptr, n, stream);
}

int lmaze_describe_reset_start(const LmazeParams* params, int64_t n, int32_t row_mode, char* text_host, int32_t len) {
    int rc = check_grid_params(params, n, TAKES_BOTH, false);
    if (!rc) rc = check_row_mode(params, row_mode, 0);
    if (rc) return rc;
    if (!text_host || len < 1) return LMAZE_E_NULL;
    text_host[0] = 0;
    if (n == 0) return 0;
    LaunchInfo info;
    memset(&info, 0, sizeof(info));
    ResetStartArgs a;
    memset(&a, 0, sizeof(a));
    a.r.n = n;
    a.r.grid = params->grid;
    a.row_mode = row_mode;
    rc = (int)launch_reset_start(params->variant, a, params->layout_mode, nullptr, &info);
    if (rc) return rc;
    return format_launch(info, text_host, len);
}

int lmaze_episode_stats(const uint8_t* done, const float* reward, const int32_t* step_count,
                        const int32_t* goal_count, float reward_goal, int64_t n, int64_t* out4, void* stream) {
    if (!done || !reward || !step_count || !out4) return LMAZE_E_NULL;
    if (n < 0 || n > LMAZE_MAX_ENVS) return LMAZE_E_COUNT;
    if (misaligned(out4, 8)) return LMAZE_E_ALIGN;
    return (int)launch_episode_stats(done, reward, step_count, goal_count, reward_goal, n, out4, (hipStream_t)stream);
}

int lmaze_bandwidth_probe(const void* src, void* dst, int64_t bytes, void* stream) {
    if (!dst) return LMAZE_E_NULL;
    if (bytes < 0 || bytes > ((int64_t)1 << 36) || (bytes & 15)) return LMAZE_E_COUNT;
    if (misaligned(dst, 16) || (src && misaligned(src, 16))) return LMAZE_E_ALIGN;
    return (int)launch_probe(src, dst, bytes, (hipStream_t)stream);
}

int lmaze_render_expanded(const int32_t* obs, int32_t grid, int32_t expansion, const int32_t* channel_mask_host,
                          int32_t channels, float* out, int64_t n, void* stream) {
    if (!obs || !channel_mask_host || !out) return LMAZE_E_NULL;
    if (grid < 1 || grid > LMAZE_MAX_GRID) return LMAZE_E_GRID;
    if (expansion < 1 || expansion > 16 || channels < 1 || channels > LMAZE_MAX_CHANNELS) return LMAZE_E_EXPANSION;
    if (n < 0 || n > LMAZE_MAX_ENVS) return LMAZE_E_COUNT;
    if (misaligned(out, 16) || misaligned(obs, 4)) return LMAZE_E_ALIGN;
    ExpandArgs a;
    a.obs = obs;
    a.out = out;
    a.n = n;
    a.grid = grid;
    a.expansion = expansion;
    a.channels = channels;
    a.chunk_floats = 0;   // chosen by the launcher, like the reciprocals
    a.inv_l = a.inv_cells = 0;
    for (int c = 0; c < LMAZE_MAX_CHANNELS; ++c) a.mask[c] = c < channels ? channel_mask_host[c] : 0;
    return (int)launch_expand(a, (hipStream_t)stream);
}

}  // extern "C"
