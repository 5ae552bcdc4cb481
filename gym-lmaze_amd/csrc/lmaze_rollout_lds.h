// The LDS layout of the workgroup rollout kernels (bodies 2-4 of lmaze_rollout_body.h), one text for both sides: the kernels
// take their pointers from these offsets, rollout_plan (lmaze_step.hip) the bytes a launch requests, and a host-compiled
// program (tests/csrc/rollout_lds_host.cpp, rollout_lds_env_host.cpp; CPU suite) writes every array's whole extent into
// exactly `total` bytes under the sanitizers.  Plain integers; cells = G * G, epb = envs per workgroup.
#ifndef LMAZE_ROLLOUT_LDS_H_
#define LMAZE_ROLLOUT_LDS_H_
#ifndef LMAZE_HD
#ifdef __HIPCC__
#define LMAZE_HD __host__ __device__ __forceinline__
#else
#define LMAZE_HD static inline
#endif
#endif

// What sits behind a body's own arrays: nothing (open loop), the epsilon-greedy byte table -- reserved in every shape, for
// the goal-keyed table too, which is read from global memory: one size per shape --, the sampling thresholds staged (one
// 16-byte row per cell, from the first 16-byte boundary on) or left in global memory (nothing reserved); and, body 3 only,
// the byte tables of the workgroup's own envs (lmaze_env_rollout_policy: one table per env, uint8[epb * cells] copied by
// dwords as the layouts are, from the first 16-byte boundary behind them on).  Every other per-env-table form reads its
// table from global memory and takes LMAZE_TAB_GLOBAL.
enum { LMAZE_TAB_NONE = 0, LMAZE_TAB_BYTES = 1, LMAZE_TAB_ROWS = 2, LMAZE_TAB_GLOBAL = 3, LMAZE_TAB_ENV_BYTES = 4 };

// Byte offsets from the start of dynamic LDS, the same under every table kind but for tab, and the bytes to request.  pat:
// int[cells], u8 (patw) uint32[4][pw]; ballflat, goalflat: int[epb], u8 [epb + 1]; lay: uint8[cells], per-env (lays)
// uint8[epb * cells] copied by dwords; spawn: uint16[cells]; tab: uint8[cells] or 16-byte rows [cells] -- with
// LMAZE_TAB_GLOBAL where the rows would start (the kernels form the pointer and never follow it); LMAZE_TAB_ENV_BYTES (body 3):
// uint8[epb * cells].  Not in the body: 0.
struct LmazeRolloutLds { int pat, ballflat, goalflat, lay, spawn, tab, total; };

LMAZE_HD int lmaze_lds_up16(int x) { return (x + 15) & ~15; }
LMAZE_HD int lmaze_rollout_u8_pw(int cells) { return (2 * cells + 16 + 3) >> 2; }   // dwords of one shifted pattern copy

// The table behind `end` bytes of arrays.  rounded (u8): the sum is rounded even where the byte table starts at `end`.
LMAZE_HD LmazeRolloutLds lmaze_rollout_lds_tab(LmazeRolloutLds l, int end, bool rounded, int cells, int kind) {
    const bool rows = kind == LMAZE_TAB_ROWS || kind == LMAZE_TAB_GLOBAL;
    l.tab = rows ? lmaze_lds_up16(end) : end;
    l.total = rows ? l.tab + (kind == LMAZE_TAB_ROWS ? 16 * cells : 0)
                   : (rounded ? lmaze_lds_up16(end) : end) + (kind == LMAZE_TAB_BYTES ? lmaze_lds_up16(cells) : 0);
    return l;
}

LMAZE_HD LmazeRolloutLds lmaze_rollout_lds_shared(int cells, int epb, int kind) {   // rollout_shared_kernel (body 2)
    LmazeRolloutLds l = {0, cells * 4, cells * 4 + epb * 4, cells * 4 + epb * 8, 0, 0, 0};
    l.spawn = l.lay + lmaze_lds_up16(cells);
    return lmaze_rollout_lds_tab(l, l.spawn + lmaze_lds_up16(cells * 2), false, cells, kind);
}
LMAZE_HD LmazeRolloutLds lmaze_rollout_lds_perenv(int cells, int epb, int kind) {   // rollout_perenv_kernel (body 3)
    LmazeRolloutLds l = {0, 0, epb * 4, epb * 8, 0, 0, 0};
    const int end = l.lay + lmaze_lds_up16(epb * cells);
    if (kind != LMAZE_TAB_ENV_BYTES) return lmaze_rollout_lds_tab(l, end, false, cells, kind);
    l.tab = lmaze_lds_up16(end);                       // a table per env: as many bytes again as the layouts
    l.total = l.tab + lmaze_lds_up16(epb * cells);
    return l;
}
LMAZE_HD LmazeRolloutLds lmaze_rollout_lds_u8(int cells, int epb, int kind) {       // rollout_shared_u8_kernel (body 4)
    LmazeRolloutLds l = {0, 4 * lmaze_rollout_u8_pw(cells) * 4, 0, 0, 0, 0, 0};
    l.goalflat = l.ballflat + (epb + 1) * 4;
    l.spawn = l.goalflat + (epb + 1) * 4;
    l.lay = l.spawn + ((cells + 1) & ~1) * 2;
    return lmaze_rollout_lds_tab(l, l.lay + cells, true, cells, kind);
}

#endif  // LMAZE_ROLLOUT_LDS_H_
